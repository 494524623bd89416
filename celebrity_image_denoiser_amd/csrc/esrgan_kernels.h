// esrgan_kernels.h — gfx950 device kernels of the server's ESRGANGenerator forward (cid_esr_forward, include/cid.h),
// reference backend/app.py:188-218, eval mode, fp32.
//
//     x1  = PReLU(Conv2d(3, 64, 9, pad 4)(x))                                 k_esr_head
//     x  <- x + BN(Conv3x3(PReLU(BN(Conv3x3(x)))))      R residual blocks     k_esr_conv<EPI>, two launches per block
//     out = Conv2d(64, 3, 9, pad 4)(x1 + x2)                                  k_esr_tail
//
// Activations between launches are fp32 in the C8 layout of disc_kernels.h: element (n, c, y, x) of a 64-channel H x W tensor is at
//     (((n * 8 + c/8) * H + y) * W + x) * 8 + c % 8.
//   * k_esr_head<U8>: the 9x9 3 -> 64 convolution + bias + PReLU on the VALU, one thread per pixel with the 64 channel sums in
//     registers; the K = 243 weights are wave-uniform and come through scalar loads.  It reads fp32 [N,3,H,W] or uint8 [N,H,W,3]
//     as (float)u / 255.0f (a true division) and writes x1; with R = 0 it also writes x1 + x1, the tensor the tail reads then.
//     k_esr_head<U8, true> also stores the sums before PReLU (cid_esr_forward_saved).
//   * k_esr_conv<EPI>: the 3x3 64 -> 64 convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32), in the tiling of
//     k_disc_conv<64, 64, 1> (a 256-thread workgroup owns 16 x 16 output pixels and all 64 channels; weights are the A operand,
//     so a lane's four accumulators are four consecutive channels of one pixel and leave as one 16-byte store).  BatchNorm uses
//     the running statistics folded into (s, t) on the host: y = fmaf(s, conv + bias, t).  Epilogues:
//         EPI_PRELU  out = prelu(y)                 block.0-2
//         EPI_RES    out = res + y                  block.3-4 (res = the block's input; out may be the same buffer)
//         EPI_SUM    out = x1 + (res + y)           block.3-4 of the last block: the tensor the tail reads
//         EPI_BN     out = y                        the SRGAN generator's blocks, which have no skip (srgan_kernels.h)
//     PReLU is v > 0 ? v : a * v (a learned slope may be negative or above 1).  Halo positions outside the image are zero.
//   * k_esr_tail<U8>: the 9x9 64 -> 3 convolution + bias on the VALU.  COUT = 3 would fill 3 of an MFMA tile's 16 rows, so the
//     kernel keeps 8 consecutive pixels x 3 channels in registers per thread instead: one 16-float row segment read from LDS
//     feeds 216 FMAs.  A 128-thread workgroup owns 16 x 64 output pixels; the contraction runs over 4-channel chunks whose halo
//     (24 x 72) is staged global -> LDS planes.  It writes fp32 [N,3,H,W], or uint8 [N,H,W,3] as clamp(0,1) * 255 truncated.
// Every sum has a fixed order (chunk, channel, kh, kw; the tail adds each 4-channel chunk's partial sum to its total) and an image's tiles depend only on (H, W), never on N or on its position
// in the batch.  No atomics.  Offsets are 64-bit; only a pixel index inside one image is an int (H * W < 2^31 is checked on the host).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "disc_kernels.h"

namespace cid {

typedef __attribute__((address_space(4))) const float* EsrConstF;   // uniform addresses here become scalar loads

__device__ __forceinline__ float e_prelu(float v, float a) { return v > 0.0f ? v : a * v; }

// ---------------------------------------------------------------------------------------------------------------------------
// Head: Conv2d(3, 64, 9, padding=4) + bias + PReLU -> x1 (C8).
constexpr int E_HEAD_K = 243;
struct EsrHeadArgs {
    const void* in;     // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    float* x1;          // C8
    float* twice;       // R = 0: x1 + x1 goes here too (the tail's input); else null
    const float* w;     // [243 = (ci, kh, kw)][64 co], then the 64 biases, then the slope
    int H, W;
    int n0;             // first image of this launch (grid y = image - n0)
};

// SAVE (cid_esr_forward_saved): the sums before PReLU go to a.pre as well, x1's layout; the backward's mask and slope gradient need them.
struct EsrHeadSavedArgs : EsrHeadArgs {
    float* pre;
};

template <bool U8, bool SAVE = false>
__global__ void __launch_bounds__(D_THREADS) k_esr_head(const std::conditional_t<SAVE, EsrHeadSavedArgs, EsrHeadArgs> a) {
    const int p = blockIdx.x * D_THREADS + threadIdx.x;
    const long long HW = (long long)a.H * a.W;
    if (p >= HW) return;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int y = p / a.W, x = p - y * a.W;
    const EsrConstF wc = (EsrConstF)a.w;
    float acc[64];
#pragma unroll
    for (int c = 0; c < 64; ++c) acc[c] = wc[E_HEAD_K * 64 + c];
    for (int ci = 0; ci < 3; ++ci)
        for (int kh = 0; kh < 9; ++kh) {
            const int iy = y + kh - 4;
            const bool row_ok = iy >= 0 && iy < a.H;
            float v[9];
#pragma unroll
            for (int kw = 0; kw < 9; ++kw) {
                const int ix = x + kw - 4;
                v[kw] = 0.0f;
                if (row_ok && ix >= 0 && ix < a.W) {
                    const size_t pix = (size_t)iy * a.W + ix;
                    if (U8) v[kw] = (float)static_cast<const unsigned char*>(a.in)[(n * HW + pix) * 3 + ci] / 255.0f;
                    else v[kw] = static_cast<const float*>(a.in)[(n * 3 + ci) * HW + pix];
                }
            }
            const EsrConstF wk = wc + (ci * 9 + kh) * 9 * 64;
#pragma unroll
            for (int kw = 0; kw < 9; ++kw)
#pragma unroll
                for (int c = 0; c < 64; ++c) acc[c] = fmaf(wk[kw * 64 + c], v[kw], acc[c]);
        }
    const float slope = wc[E_HEAD_K * 64 + 64];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = e_prelu(acc[cb * 8 + j], slope);
        const size_t at = ((n * 8 + cb) * HW + p) * 8;
        d_f32x4* o = reinterpret_cast<d_f32x4*>(a.x1 + at);
        o[0] = d_f32x4{v[0], v[1], v[2], v[3]};
        o[1] = d_f32x4{v[4], v[5], v[6], v[7]};
        if (a.twice) {
            d_f32x4* o2 = reinterpret_cast<d_f32x4*>(a.twice + at);
            o2[0] = d_f32x4{v[0] + v[0], v[1] + v[1], v[2] + v[2], v[3] + v[3]};
            o2[1] = d_f32x4{v[4] + v[4], v[5] + v[5], v[6] + v[6], v[7] + v[7]};
        }
        if constexpr (SAVE) {
            d_f32x4* q = reinterpret_cast<d_f32x4*>(a.pre + at);
            q[0] = d_f32x4{acc[cb * 8], acc[cb * 8 + 1], acc[cb * 8 + 2], acc[cb * 8 + 3]};
            q[1] = d_f32x4{acc[cb * 8 + 4], acc[cb * 8 + 5], acc[cb * 8 + 6], acc[cb * 8 + 7]};
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Trunk: 3x3 convolution 64 -> 64, padding 1, as an implicit GEMM on v_mfma_f32_16x16x4_f32, BatchNorm (running statistics) and
// one of three epilogues.
constexpr int E_CONV_W = 64 * 64 * 9;   // packed weights of one trunk convolution
// one trunk segment of the blob: weights, then bias[64], s[64], t[64], slope
constexpr int E_CONV_BIAS = E_CONV_W, E_CONV_S = E_CONV_W + 64, E_CONV_T = E_CONV_W + 128, E_CONV_SLOPE = E_CONV_W + 192;
enum { EPI_PRELU = 0, EPI_RES = 1, EPI_SUM = 2, EPI_BN = 3 };

struct EsrConvArgs {
    const float* in;      // C8, 64 channels
    float* out;           // C8, 64 channels
    const float* res;     // EPI_RES / EPI_SUM: the block's input (may be `out`: a position is read before it is written, by the same lane)
    const float* x1;      // EPI_SUM
    const float* w;       // packed [8 chunks][9 taps][8][64] (DiscConvArgs::w), then bias, s, t, slope
    int H, W;
    int tiles_x;          // tiles per tile row
    int n0;
};

template <int EPI>
__global__ void __launch_bounds__(D_THREADS, 2) k_esr_conv(const EsrConvArgs a) {
    using G = DiscGeom<64, 64, 1>;
    constexpr int TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];

    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int iy0 = ty * TH - 1, ix0 = tx * D_TW - 1;
    const size_t plane = (size_t)a.H * a.W;

    d_f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * 4) * HWD + l16;   // this lane's B operand base (plane kq, its pixel column)
    const int wb = kq * WSTR + l16;                    // this lane's A operand base (row kq, its channel)

    for (int chunk = 0; chunk < 8; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk
        // ---- halo of this chunk: global -> VGPR -> LDS planes; outside the image: the convolution's zero padding
        const float* src = a.in + ((n * 8 + chunk) * plane) * 8;
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int iy = iy0 + hy, ix = ix0 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    v = *reinterpret_cast<const d_f32x4*>(src + ((size_t)iy * a.W + ix) * 8 + h * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights: 72 rows (tap, channel) of 64
        const float* wsrc = a.w + (size_t)chunk * 72 * 64;
        for (int i = tid; i < 72 * 16; i += D_THREADS) {
            const int r = i >> 4, c4 = i & 15;
            *reinterpret_cast<d_f32x4*>(&lds_w[r * WSTR + c4 * 4]) = *reinterpret_cast<const d_f32x4*>(wsrc + r * 64 + c4 * 4);
        }
        __syncthreads();
        // ---- 9 taps x 2 k-steps of 4 channels: 16 MFMAs per k-step per wave
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap % 3;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                float av[4], bv[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) av[ct] = lds_w[wb + (tap * 8 + sub * 4) * WSTR + ct * 16];
#pragma unroll
                for (int pt = 0; pt < 4; ++pt) bv[pt] = lds_x[xb + sub * 4 * XSTR + (pt + kh) * HWD + kw];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: + bias, BatchNorm, then PReLU or the residual sums; four consecutive channels of one pixel per lane
    const int ox = tx * D_TW + l16;
    const float slope = a.w[E_CONV_SLOPE];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int co = ct * 16 + kq * 4;   // first of this lane's four channels
        const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(a.w + E_CONV_BIAS + co);
        const d_f32x4 s4 = *reinterpret_cast<const d_f32x4*>(a.w + E_CONV_S + co);
        const d_f32x4 t4 = *reinterpret_cast<const d_f32x4*>(a.w + E_CONV_T + co);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const int oy = ty * TH + wm * 4 + pt;
            if (oy < a.H && ox < a.W) {
                const size_t at = (((n * 8 + co / 8) * a.H + oy) * (size_t)a.W + ox) * 8 + (co & 7);
                const d_f32x4 z = acc[ct][pt] + b4;
                d_f32x4 y;
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = d_bn(s4[r], z[r], t4[r]);
                if (EPI == EPI_PRELU) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) y[r] = e_prelu(y[r], slope);
                } else if (EPI != EPI_BN) {
                    y = *reinterpret_cast<const d_f32x4*>(a.res + at) + y;
                    if (EPI == EPI_SUM) y = *reinterpret_cast<const d_f32x4*>(a.x1 + at) + y;
                }
                *reinterpret_cast<d_f32x4*>(a.out + at) = y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tail: Conv2d(64, 3, 9, padding=4) + bias -> fp32 [N,3,H,W], or the server's uint8 view clamp(0,1) * 255 truncated, [N,H,W,3].
constexpr int E_TAIL_THREADS = 128;
constexpr int E_TAIL_TH = 16, E_TAIL_TW = 64, E_TAIL_PX = 8;         // tile rows / columns, pixels per thread (one row segment)
constexpr int E_TAIL_HH = E_TAIL_TH + 8, E_TAIL_HW = E_TAIL_TW + 8;  // halo
constexpr int E_TAIL_RS = E_TAIL_HW + 4;                             // LDS row stride (16-byte aligned rows)
constexpr int E_TAIL_PLANE = E_TAIL_HH * E_TAIL_RS;
constexpr int E_TAIL_WROW = 32;                                      // floats per (ci, kh) weight row: [co][kw] = 27, padded
constexpr int E_TAIL_W = 64 * 9 * E_TAIL_WROW;

struct EsrTailArgs {
    const float* in;    // C8, 64 channels: x1 + x2
    void* out;          // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    const float* w;     // [64 ci][9 kh][32: co * 9 + kw], then the 3 biases
    int H, W;
    int tiles_x;
    int n0;
};

// The convolution itself, shared with the SRGAN generator's tail (srgan_kernels.h): acc[co][j] = bias + the 5184-term sum of output
// pixel (ty * 16 + ry, tx * 64 + cx + j), channel co.  `lds` holds 4 * E_TAIL_PLANE floats.
__device__ __forceinline__ void e_tail_sums(const EsrTailArgs& a, float* lds, int ty, int tx, size_t n, float (&acc)[3][E_TAIL_PX]) {
    const int tid = threadIdx.x;
    const int ry = tid >> 3, cx = (tid & 7) * E_TAIL_PX;   // this thread's row and first column inside the tile
    const int iy0 = ty * E_TAIL_TH - 4, ix0 = tx * E_TAIL_TW - 4;
    const size_t plane = (size_t)a.H * a.W;
    const EsrConstF wc = (EsrConstF)a.w;

#pragma unroll
    for (int co = 0; co < 3; ++co)
#pragma unroll
        for (int j = 0; j < E_TAIL_PX; ++j) acc[co][j] = wc[E_TAIL_W + co];

    for (int chunk = 0; chunk < 16; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk
        // ---- halo of channels 4*chunk .. 4*chunk+3: one 16-byte load per pixel -> four LDS planes; outside the image: zero
        const float* src = a.in + ((n * 8 + (chunk >> 1)) * plane) * 8 + (chunk & 1) * 4;
        for (int idx = tid; idx < E_TAIL_HH * E_TAIL_HW; idx += E_TAIL_THREADS) {
            const int hy = idx / E_TAIL_HW, hx = idx - hy * E_TAIL_HW;
            const int iy = iy0 + hy, ix = ix0 + hx;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = *reinterpret_cast<const d_f32x4*>(src + ((size_t)iy * a.W + ix) * 8);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds[j * E_TAIL_PLANE + hy * E_TAIL_RS + hx] = v[j];
        }
        __syncthreads();
        // this chunk's 324 terms are summed on their own and then added to the total: a shorter rounding chain than 5184 in a row
        float part[3][E_TAIL_PX];
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int j = 0; j < E_TAIL_PX; ++j) part[co][j] = 0.0f;
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
#pragma unroll 1
            for (int kh = 0; kh < 9; ++kh) {
                float in[E_TAIL_PX + 8];
                const float* row = &lds[c * E_TAIL_PLANE + (ry + kh) * E_TAIL_RS + cx];
#pragma unroll
                for (int q = 0; q < (E_TAIL_PX + 8) / 4; ++q) {
                    const d_f32x4 v = *reinterpret_cast<const d_f32x4*>(row + q * 4);
                    in[q * 4] = v[0];
                    in[q * 4 + 1] = v[1];
                    in[q * 4 + 2] = v[2];
                    in[q * 4 + 3] = v[3];
                }
                const EsrConstF wk = wc + ((chunk * 4 + c) * 9 + kh) * E_TAIL_WROW;
#pragma unroll
                for (int kw = 0; kw < 9; ++kw)
#pragma unroll
                    for (int co = 0; co < 3; ++co) {
                        const float wv = wk[co * 9 + kw];
#pragma unroll
                        for (int j = 0; j < E_TAIL_PX; ++j) part[co][j] = fmaf(wv, in[j + kw], part[co][j]);
                    }
            }
        }
#pragma unroll
        for (int co = 0; co < 3; ++co)
#pragma unroll
            for (int j = 0; j < E_TAIL_PX; ++j) acc[co][j] += part[co][j];
    }
}

template <bool U8>
__global__ void __launch_bounds__(E_TAIL_THREADS) k_esr_tail(const EsrTailArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[4 * E_TAIL_PLANE];
    const int tid = threadIdx.x;
    const int ry = tid >> 3, cx = (tid & 7) * E_TAIL_PX;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const size_t plane = (size_t)a.H * a.W;
    float acc[3][E_TAIL_PX];
    e_tail_sums(a, lds, ty, tx, n, acc);

    const int oy = ty * E_TAIL_TH + ry;
    if (oy >= a.H) return;
#pragma unroll
    for (int j = 0; j < E_TAIL_PX; ++j) {
        const int ox = tx * E_TAIL_TW + cx + j;
        if (ox < a.W) {
            const size_t pix = (size_t)oy * a.W + ox;
#pragma unroll
            for (int co = 0; co < 3; ++co) {
                if (U8) {
                    const float v = fminf(fmaxf(acc[co][j], 0.0f), 1.0f) * 255.0f;   // clamp(0, 1).mul(255).byte(): truncation
                    static_cast<unsigned char*>(a.out)[(n * plane + pix) * 3 + co] = (unsigned char)(int)v;
                } else {
                    static_cast<float*>(a.out)[(n * 3 + co) * plane + pix] = acc[co][j];
                }
            }
        }
    }
}

}  // namespace cid
