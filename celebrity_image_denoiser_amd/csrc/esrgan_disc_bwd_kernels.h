// esrgan_disc_bwd_kernels.h — gfx950 device kernels of the ESRGAN trainer's discriminator backward pass (cid_esd_backward,
// include/cid.h): the gradients of conv1 ... conv4 and fc (reference backend/trainingcode/esrgan_code/models.py:36-71) from
// grad_logit[N] and the four ACTIVATED tensors a1 ... a4 that cid_esd_forward_saved kept.
//
// Tensors are fp32 in the forward's C8 layout.  There is no BatchNorm, so the gradient with respect to a convolution's raw output is
//     dz = up * (a > 0 ? 1 : 0.2)
// with `a` the saved activated tensor (LeakyReLU keeps the sign, so a > 0 is the forward's decision) and `up` the gradient of `a`.
// dz is never stored: the weight- and data-gradient kernels form it while they stage their operand.  For conv4 `up` is not stored
// either: the linear layer's gradient of a4 is the rank-one dl[n] * w_c8[f] (f the C8 position inside one image, which is the order
// of the packed fc.weight), formed in the same staging (FC = true), as D_UP_HEAD does in disc_bwd_kernels.h.
//   * k_esd_fc_bwd: dW_fc[c*P + p] = sum_n dl[n] * a4[n][c8(c, p)] with fp64 products and sum, n in index order, written in the
//     reference's NCHW-flatten order; db_fc = sum_n dl[n].
//   * k_esd_wgrad<CD, CX, FC>: weight gradient of conv2, conv3, conv4 as a GEMM [CD] x [9 * 16] contracted over pixels on
//     v_mfma_f32_16x16x4_f32, in the arrangement of k_disc_wgrad at S = 2: a workgroup owns CD dz channels (grid z = part), 16 input
//     channels (grid y) and a contiguous range of (image, 4 x 16 pixel tile) items (grid x = split); it writes its own partial tile and
//     k_disc_wgrad_reduce sums the partials in fp64 in split order.  The workgroups of channel block 0 sum dz per channel in fp64:
//     the bias gradient.
//   * k_esd_dgrad<CD, CX, CXW, PT, FC>: data gradient of conv4, conv3, conv2 in gather form over the four parity classes of INPUT
//     pixels (k_disc_dgrad, S = 2): a workgroup owns a (4 / (CXW / 64) * PT) x 16 tile of one class and CXW of the CX input channels
//     (grid z = class + 4 * channel part), so every element of the activation gradient is stored exactly once.  It reads the
//     forward's packed blob, [CX/8][9][8][64] per 64-channel part of dz, transposed in staging.
//   * k_esd_wgrad1<U8> / k_esd_dgrad1: conv1 (K = 27, stride 2) on the VALU, after k_disc_wgrad0 / k_disc_dgrad0: per-workgroup fp64
//     partials summed by k_disc_wgrad0_reduce; the input gradient as a gather, one thread per input pixel of one parity class.
//   * k_esd_pack: the forward's blob from the ten parameter tensors in device memory, fc.weight's C8 permutation included.
// Every reduction across workgroups is fp64 in a fixed order; no atomics.  Offsets are 64-bit; only a pixel index inside one image
// is an int.  Every __syncthreads() is in workgroup-uniform control flow, and every LDS element that is read is written first
// (positions outside the image as 0).
#pragma once
#include "disc_bwd_kernels.h"
#include "esrgan_disc_kernels.h"

namespace cid {

// Where dz comes from.
struct EsdDzSrc {
    const float* a;      // C8: the saved activated output of this convolution
    const float* up;     // C8, same shape: gradient of `a` (unused with FC)
    const float* dl;     // FC: grad_logit [N]
    const float* wfc;    // FC: fc.weight in C8 order (the packed blob's segment)
    size_t img;          // FC: elements of `a` per image
};

// Four consecutive channels of dz at element offset `off` (a multiple of 4) of image n.
template <bool FC>
__device__ __forceinline__ d_f32x4 e_load_dz(const EsdDzSrc& s, size_t n, size_t off) {
    const d_f32x4 y = *reinterpret_cast<const d_f32x4*>(s.a + off);
    d_f32x4 u;
    if (FC) {
        const float dl = s.dl[n];
        const d_f32x4 w = *reinterpret_cast<const d_f32x4*>(s.wfc + (off - n * s.img));
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = dl * w[j];
    } else {
        u = *reinterpret_cast<const d_f32x4*>(s.up + off);
    }
    d_f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = u[j] * d_slope(y[j]);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// fc.  One thread per feature, in C8 order.
struct EsdFcBwdArgs {
    const float* a4;     // C8, 512 channels, P pixels per image
    const float* dl;     // grad_logit [N]
    float* dw;           // out [512 * P] in NCHW-flatten order, may be null
    float* db;           // out [1], may be null
    long long F, P;      // F = 512 * P
    long long N;
};

__global__ void __launch_bounds__(D_THREADS) k_esd_fc_bwd(const EsdFcBwdArgs a) {
    const long long q = (long long)blockIdx.x * D_THREADS + threadIdx.x;
    if (a.db && q == 0) {
        double s = 0.0;
        for (long long n = 0; n < a.N; ++n) s += (double)a.dl[n];
        a.db[0] = (float)s;
    }
    if (!a.dw || q >= a.F) return;
    double s = 0.0;
    for (long long n = 0; n < a.N; ++n) s += (double)a.dl[n] * (double)a.a4[(size_t)n * (size_t)a.F + (size_t)q];
    const long long j = q & 7, t = q >> 3, p = t % a.P, cb = t / a.P;
    a.dw[(size_t)((cb * 8 + j) * a.P + p)] = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Weight gradient of conv2, conv3, conv4: dW[co, ci, kh, kw] = sum_{n, oy, ox} dz[n, co, oy, ox] * ain[n, ci, 2*oy+kh-1, 2*ox+kw-1].
struct EsdWgradArgs {
    EsdDzSrc dz;
    const float* ain;      // C8, CX channels, Hin x Win: the activated input of this convolution
    float* part;           // out: part[(((split*(CX/16) + block)*CD_TOTAL + co)*9 + tap)*16 + ci%16]
    double* part_b;        // out: part_b[split*CD_TOTAL + co] (written by channel block 0)
    long long items;       // N * tiles
    int splits;
    int cd_total;          // dz channels of the layer (grid z * CD)
    int Hin, Win, Ho, Wo;
    int tiles_x, tiles;
};

// Known limit, open ("fp32 weight-gradient chains that grow with N"): a workgroup's whole range of items is one
// fp32 accumulation chain, as k_disc_wgrad's was before D_WG_CHUNK (disc_bwd_kernels.h); no test runs it at an N where that shows.
template <int CD, int CX, bool FC>
__global__ void __launch_bounds__(D_THREADS, 2) k_esd_wgrad(const EsdWgradArgs a) {
    using G = DiscWgradGeom<2>;
    constexpr int HH = G::HH, HWD = G::HWD, RS = G::RS, XSTR = G::XSTR, ZSTR = G::ZSTR;
    constexpr int RT = CD / 64;   // 16-channel row tiles per wave
    static_assert(CD == 64 || CD == 128, "one or two row tiles per wave");
    static_assert(CX % 16 == 0, "16-channel blocks");
    __shared__ float lds_a[16 * XSTR];
    __shared__ float lds_z[CD * ZSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x, blk = blockIdx.y;
    const long long it0 = a.items * split / a.splits, it1 = a.items * (split + 1) / a.splits;
    const size_t in_plane = (size_t)a.Hin * a.Win, out_plane = (size_t)a.Ho * a.Wo;
    const int co0 = (int)blockIdx.z * CD;   // first dz channel of this part

    d_f32x4 acc[RT][9];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[r][tap] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    double bsum = 0.0;

    const int zb = ((wave * RT) * 16 + l16) * ZSTR + kq * D_TW;
    const int ab = l16 * XSTR + kq * 2 * RS;

    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.tiles);
        const int t = (int)(item - (long long)n * a.tiles), ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const int oy0 = ty * D_WG_TH, ox0 = tx * D_TW;
        const int iy0 = oy0 * 2 - 1, ix0 = ox0 * 2 - 1;
        __syncthreads();   // every wave is done with the previous item
        // ---- dz tile: CD channels x 4 x 16 pixels (0 outside the tensor)
        for (int idx = tid; idx < CD * 16; idx += D_THREADS) {
            const int h = idx & 1, c = (idx >> 1) & 15, r = (idx >> 5) & 3, cb = idx >> 7;
            const int oy = oy0 + r, ox = ox0 + c;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (oy < a.Ho && ox < a.Wo)
                v = e_load_dz<FC>(a.dz, n, ((n * (size_t)(a.cd_total / 8) + co0 / 8 + cb) * out_plane + (size_t)oy * a.Wo + ox) * 8 + h * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_z[(cb * 8 + h * 4 + j) * ZSTR + r * D_TW + c] = v[j];
        }
        // ---- halo of the 16 input channels of this block (0 outside the image)
        for (int idx = tid; idx < HH * HWD * 4; idx += D_THREADS) {
            const int q = idx / (HH * HWD), p = idx - q * (HH * HWD), cb2 = q >> 1, h = q & 1;
            const int hy = p / HWD, hx = p - hy * HWD;
            const int iy = iy0 + hy, ix = ix0 + hx;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win)
                v = *reinterpret_cast<const d_f32x4*>(a.ain + ((n * (CX / 8) + blk * 2 + cb2) * in_plane + (size_t)iy * a.Win + ix) * 8 + h * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_a[(cb2 * 8 + h * 4 + j) * XSTR + hy * RS + hx] = v[j];
        }
        __syncthreads();
        if (blk == 0 && tid < CD) {
            double s = 0.0;
            for (int i = 0; i < D_WG_TH * D_TW; ++i) s += (double)lds_z[tid * ZSTR + i];
            bsum += s;
        }
        // ---- 16 k-steps (columns) of four pixel rows: RT x 9 MFMAs per step per wave
#pragma unroll 4
        for (int col = 0; col < D_TW; ++col) {
            float av[RT];
#pragma unroll
            for (int r = 0; r < RT; ++r) av[r] = lds_z[zb + r * 16 * ZSTR + col];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float bv = lds_a[ab + (tap / 3) * RS + col * 2 + tap % 3];
#pragma unroll
                for (int r = 0; r < RT; ++r) acc[r][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv, acc[r][tap], 0, 0, 0);
            }
        }
    }

    // a lane holds dz channels 4*kq .. 4*kq+3 of its row tile for input channel l16
    float* part = a.part + (((size_t)split * (CX / 16) + blk) * a.cd_total + co0) * 144;
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int co = (wave * RT + r) * 16 + kq * 4 + e;
                part[((size_t)co * 9 + tap) * 16 + l16] = acc[r][tap][e];
            }
    if (blk == 0 && tid < CD) a.part_b[(size_t)split * a.cd_total + co0 + tid] = bsum;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Data gradient of conv4, conv3, conv2 (3x3, stride 2, pad 1): out[n, ci, iy, ix] = sum_{co, kh, kw} dz[n, co, oy, ox] * W[co, ci, kh, kw]
// with iy = 2*oy + kh - 1.  In class coordinates (iy = 2*i + py, ix = 2*j + px) the taps of a class read dz at (i + d, j + e), d, e in
// {0, 1}: py = 0: kh = 1, d = 0;  py = 1: kh = 0, d = 1 and kh = 2, d = 0 (k_disc_dgrad, S = 2).
struct EsdDgradArgs {
    EsdDzSrc dz;
    const float* w;       // the forward's packed weights of this layer: per 64 dz channels [CX/8][9 taps][8][64], then their biases
    float* out;           // C8, CX channels, Hin x Win
    int Hin, Win, Ho, Wo;
    int tiles_x;          // tiles per tile row of class (0, 0), the largest class
    int n0;
};

template <int CXW, int PT>
struct EsdDgradGeom {
    static constexpr int WN = CXW / 64;
    static constexpr int WM = 4 / WN;
    static constexpr int TH = WM * PT;                          // class rows per tile
    static constexpr int HH = TH + 1;
    static constexpr int HWD = D_TW + 1;
    static constexpr int NPIX = HH * HWD;
    static constexpr int XSTR = NPIX + ((16 - NPIX % 32) + 32) % 32;   // 16 mod 32: planes k and k+1 on disjoint banks
    static constexpr int WSTR = CXW + 16;
    static constexpr int STAGE_ITERS = (NPIX * 2 + D_THREADS - 1) / D_THREADS;
    static_assert(CXW == 64 || CXW == 128, "64 channels per wave");
    static_assert(PT == 1 || PT == 2 || PT == 4, "rows per wave");
};

template <int CD, int CX, int CXW, int PT, bool FC>
__global__ void __launch_bounds__(D_THREADS, 2) k_esd_dgrad(const EsdDgradArgs a) {
    static_assert(CD % ESD_PART == 0 && CX % CXW == 0, "whole parts");
    using G = EsdDgradGeom<CXW, PT>;
    constexpr int WM = G::WM, TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l16 = lane & 15, kq = lane >> 4;
    const int cls = blockIdx.z & 3, py = cls >> 1, px = cls & 1;
    const int ci0 = (int)(blockIdx.z >> 2) * CXW;                        // first input channel of this workgroup
    const int Hc = (a.Hin - py + 1) / 2, Wc = (a.Win - px + 1) / 2;      // rows / columns of this class
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int i0 = ty * TH, j0 = tx * D_TW;
    if (i0 >= Hc || j0 >= Wc) return;   // the whole workgroup: a smaller class has fewer tiles
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const size_t out_plane = (size_t)a.Ho * a.Wo;
    const int ny = 1 + py, nx = 1 + px;

    d_f32x4 acc[4][PT];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * PT) * HWD + l16;
    const int wb = kq * WSTR + wn * 64 + l16;

    for (int chunk = 0; chunk < CD / 8; ++chunk) {
        __syncthreads();
        // ---- dz halo of this chunk: global (a, upstream) -> dz -> LDS planes
        const size_t src = ((n * (CD / 8) + chunk) * out_plane) * 8;
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int oy = i0 + hy, ox = j0 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (oy < a.Ho && ox < a.Wo) v = e_load_dz<FC>(a.dz, n, src + ((size_t)oy * a.Wo + ox) * 8 + h * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights, transposed: row (tap, dz channel) holds the CXW input channels
        const float* wp = a.w + (size_t)(chunk * 8 / ESD_PART) * ((size_t)CX * 9 * ESD_PART + ESD_PART) + (chunk * 8) % ESD_PART;
        for (int i = tid; i < 18 * CXW; i += D_THREADS) {
            const int cl = i % CXW, r = i / CXW, h = r & 1, tap = r >> 1, ci = ci0 + cl;
            const size_t row = (size_t)((ci >> 3) * 9 + tap) * 8 + (ci & 7);
            const d_f32x4 v = *reinterpret_cast<const d_f32x4*>(wp + row * ESD_PART + h * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_w[(tap * 8 + h * 4 + j) * WSTR + cl] = v[j];
        }
        __syncthreads();
        for (int ay = 0; ay < ny; ++ay) {
            const int kh = py ? 2 * ay : 1;
            const int dy = py ? 1 - ay : 0;    // halo row of the tile's row 0 for this tap
            for (int ax = 0; ax < nx; ++ax) {
                const int kw = px ? 2 * ax : 1;
                const int dx = px ? 1 - ax : 0;
                const int tap = kh * 3 + kw;
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    float av[4], bv[PT];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) av[ct] = lds_w[wb + (tap * 8 + sub * 4) * WSTR + ct * 16];
#pragma unroll
                    for (int pt = 0; pt < PT; ++pt) bv[pt] = lds_x[xb + sub * 4 * XSTR + (pt + dy) * HWD + dx];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
                }
            }
        }
    }

    const int j = j0 + l16;
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int i = i0 + wm * PT + pt;
        if (i < Hc && j < Wc) {
            const int iy = i * 2 + py, ix = j * 2 + px;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int ci = ci0 + wn * 64 + ct * 16 + kq * 4;
                *reinterpret_cast<d_f32x4*>(a.out + (((n * (CX / 8) + ci / 8) * a.Hin + iy) * (size_t)a.Win + ix) * 8 + (ci & 7)) = acc[ct][pt];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// conv1.  dz1 = da1 * (a1 > 0 ? 1 : 0.2) is d_dz0(a1, da1, .).
// Weight and bias gradient: dW1[co, k] = sum_{n, p} dz1[n, co, p] * patch[n, p, k], k = (ci*3 + kh)*3 + kw over the stride-2 patch of
// output pixel p, and k = 27 the constant 1 (the bias).  A workgroup walks a contiguous range of (image, 64-pixel strip) items of a1;
// thread = (channel co, group of 7 k).  The input is decoded as k_esd_conv1 decodes it.
struct EsdWgrad1Args {
    const void* in;        // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    const float* a1;
    const float* da1;
    double* part;          // out: part[(split*64 + co)*28 + k]
    long long items;       // N * strips
    int splits, strips;
    int H, W, Ho, Wo;
};

template <bool U8>
__global__ void __launch_bounds__(D_THREADS) k_esd_wgrad1(const EsdWgrad1Args a) {
    __shared__ float lds_d[64 * 64];   // [pixel][co]
    __shared__ float lds_p[64 * 28];   // [pixel][k]
    const int tid = threadIdx.x, co = tid & 63, kg = tid >> 6;
    const size_t HW = (size_t)a.H * a.W;
    const long long HWo = (long long)a.Ho * a.Wo;
    const long long it0 = a.items * blockIdx.x / a.splits, it1 = a.items * (blockIdx.x + 1) / a.splits;
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.strips);
        const long long p0 = (item - (long long)n * a.strips) * 64;
        __syncthreads();
        for (int idx = tid; idx < 64 * 16; idx += D_THREADS) {
            const int h = idx & 1, px = (idx >> 1) & 63, cb = idx >> 7;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (p0 + px < HWo) v = d_dz0(a.a1, a.da1, ((n * 8 + cb) * (size_t)HWo + (size_t)(p0 + px)) * 8 + h * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_d[px * 64 + cb * 8 + h * 4 + j] = v[j];
        }
        for (int idx = tid; idx < 64 * 28; idx += D_THREADS) {
            const int px = idx / 28, k = idx - px * 28;
            const long long p = p0 + px;
            float v = 0.0f;
            if (p < HWo) {
                if (k == 27) {
                    v = 1.0f;
                } else {
                    const int ci = k / 9, kh = (k / 3) % 3, kw = k % 3;
                    const int y = (int)(p / a.Wo), x = (int)(p - (long long)y * a.Wo);
                    const int iy = 2 * y + kh - 1, ix = 2 * x + kw - 1;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                        const size_t pix = (size_t)iy * a.W + ix;
                        if (U8) v = (float)static_cast<const unsigned char*>(a.in)[(n * HW + pix) * 3 + ci] / 255.0f;
                        else v = static_cast<const float*>(a.in)[(n * 3 + ci) * HW + pix];
                    }
                }
            }
            lds_p[idx] = v;
        }
        __syncthreads();
        for (int px = 0; px < 64; ++px) {
            const double d = (double)lds_d[px * 64 + co];
#pragma unroll
            for (int j = 0; j < 7; ++j) acc[j] += d * (double)lds_p[px * 28 + kg * 7 + j];
        }
    }
#pragma unroll
    for (int j = 0; j < 7; ++j) a.part[((size_t)blockIdx.x * 64 + co) * 28 + kg * 7 + j] = acc[j];
}

// Input gradient: dx[n, ci, y, x] = sum_{co, kh, kw} dz1[n, co, oy, ox] * W1[co, ci, kh, kw] with y = 2*oy + kh - 1, x = 2*ox + kw - 1.
// One thread per input pixel of one parity class (grid z), so a workgroup's threads share their taps.
struct EsdDgrad1Args {
    const float* a1;
    const float* da1;
    const float* w;     // [64][3][3][3]
    float* out;         // fp32 [N,3,H,W]
    int H, W, Ho, Wo;
    int n0;
};

__global__ void __launch_bounds__(D_THREADS) k_esd_dgrad1(const EsdDgrad1Args a) {
    const int cls = blockIdx.z, py = cls >> 1, px = cls & 1;
    const int Hc = (a.H - py + 1) / 2, Wc = (a.W - px + 1) / 2;
    const int p = blockIdx.x * D_THREADS + threadIdx.x;
    if (p >= Hc * Wc) return;
    const size_t HW = (size_t)a.H * a.W, HWo = (size_t)a.Ho * a.Wo;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int i = p / Wc, j = p - i * Wc;
    typedef __attribute__((address_space(4))) const float* ConstF;
    const ConstF wc = (ConstF)a.w;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int ay = 0; ay <= py; ++ay) {
        const int kh = py ? 2 * ay : 1, oy = i + (py ? 1 - ay : 0);
        if (oy >= a.Ho) continue;
        for (int ax = 0; ax <= px; ++ax) {
            const int kw = px ? 2 * ax : 1, ox = j + (px ? 1 - ax : 0);
            if (ox >= a.Wo) continue;
            const size_t pix = (size_t)oy * a.Wo + ox;
            for (int cb = 0; cb < 8; ++cb) {
                const size_t off = ((n * 8 + cb) * HWo + pix) * 8;
                const d_f32x4 d0 = d_dz0(a.a1, a.da1, off), d1 = d_dz0(a.a1, a.da1, off + 4);
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float d = q < 4 ? d0[q & 3] : d1[q & 3];
                    const int wbase = (cb * 8 + q) * 27 + kh * 3 + kw;
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) acc[ci] = fmaf(wc[wbase + ci * 9], d, acc[ci]);
                }
            }
        }
    }
    const size_t pix = (size_t)(2 * i + py) * a.W + (2 * j + px);
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) a.out[(n * 3 + ci) * HW + pix] = acc[ci];
}

// ---------------------------------------------------------------------------------------------------------------------------
// The packed blob (EsdBlob, api/esrgan_disc.h) from the ten parameter tensors in device memory: what cid_esd_set_weight x 10 builds on
// the host, byte for byte (alignment gaps are 0).  One thread per float of the blob.  conv1 keeps the reference layout; conv2 ... conv4
// are packed as k_disc_pack packs a layer in 64-channel parts; fc.weight goes from NCHW-flatten to C8 order.
struct EsdPackArgs {
    const float* w[5];
    const float* b[5];
    float* blob;
    long long off[4];     // conv1 ... conv4
    long long fcw, fcb, total;
    long long P;          // H4 * W4
};

__global__ void __launch_bounds__(D_THREADS) k_esd_pack(const EsdPackArgs a) {
    const long long i = (long long)blockIdx.x * D_THREADS + threadIdx.x;
    if (i >= a.total) return;
    float v = 0.0f;
    if (i >= a.fcb) {
        if (i == a.fcb) v = a.b[4][0];
    } else if (i >= a.fcw) {
        const long long r = i - a.fcw;
        if (r < 512 * a.P) {
            const long long j = r & 7, t = r >> 3, p = t % a.P, cb = t / a.P;
            v = a.w[4][(size_t)((cb * 8 + j) * a.P + p)];
        }
    } else {
        int l = 0;
#pragma unroll
        for (int k = 1; k < 4; ++k)
            if (i >= a.off[k]) l = k;
        const int cin = l == 0 ? 3 : 32 << l, cout = 64 << l;   // 3 -> 64 -> 128 -> 256 -> 512
        const int r = (int)(i - a.off[l]), nw = cout * cin * 9;
        if (l == 0) {
            if (r < nw) v = a.w[0][r];
            else if (r < nw + cout) v = a.b[0][r - nw];
        } else {
            const int nwp = cin * 9 * ESD_PART, block = nwp + ESD_PART;
            const int pi = r / block, rr = r - pi * block;
            if (pi < cout / ESD_PART) {
                if (rr < nwp) {
                    const int co = pi * ESD_PART + rr % ESD_PART, q = rr / ESD_PART, ci8 = q & 7, tap = (q >> 3) % 9, chunk = (q >> 3) / 9;
                    v = a.w[l][((size_t)co * cin + chunk * 8 + ci8) * 9 + tap];
                } else {
                    v = a.b[l][pi * ESD_PART + rr - nwp];
                }
            }
        }
    }
    a.blob[i] = v;
}

}  // namespace cid
