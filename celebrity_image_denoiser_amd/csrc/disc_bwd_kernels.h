// disc_bwd_kernels.h — gfx950 device kernels of the DenoiseDiscriminator backward pass (cid_disc_backward, include/cid.h): the
// gradients of model.0 ... model.13 (reference backend/trainingcode/denoise_gan_code/training.py:77-98) from grad_prob[N] and what
// cid_disc_forward_saved kept: the activated a0, the raw z2, z5, z8, each BatchNorm's (scale, shift) and (mean, invstd).
//
// Tensors are fp32 in the forward's C8 layout (disc_kernels.h).  Every reduction accumulates in fp64 in a fixed order, no atomics;
// the GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32).  An image's tiling depends only on (H, W).
//
// Per BatchNorm l the gradient with respect to the raw z is an elementwise function of (z, upstream gradient) and eight per-channel
// numbers ("coef", D_COEF floats: s, t, k = gamma*invstd, mean, invstd, m1 = dbeta/M, m2 = dgamma/M, head weight / P):
//     y = d_bn(s, z, t)         mask = y > 0 ? 1 : 0.2      g = up * mask       xh = (z - mean) * invstd
//     dz = k * (g - m1 - xh * m2)          (eval mode: m1 = m2 = 0)
// d_bn is the forward's own function, so the mask is the forward's decision bit for bit.  dz is never stored: the wgrad and dgrad
// kernels evaluate it while they stage their operand, as the forward applies BatchNorm + LeakyReLU in its staging.
//   * k_disc_head_bwd / k_disc_head_reduce: the head.  Per image the channel means of a8 (as k_disc_head computes them), the
//     probability, dl = grad_prob * p * (1 - p); then dW12[c] = sum_n dl[n] * mean[n][c], db12 = sum_n dl[n].  The gradient of a8,
//     dl[n] * w12[c] / P, is not stored either: BN9's consumers form it from dl and coef[7].
//   * k_disc_bn_bwd_part<C, HEAD> + k_disc_bn_bwd_reduce: per-workgroup fp64 sums of g and g * xh into a slab, then one workgroup
//     per channel reduces it in a fixed order, writes dgamma, dbeta and the channel's coef.
//   * k_disc_wgrad<CD, CX, S, BN_IN, HEAD>: weight gradient of layers 2, 5, 8 as a GEMM [CD] x [9 * CX] contracted over pixels.  A
//     workgroup owns 16 input channels (144 columns) and a contiguous range of (image, 4 x 16 pixel tile) items; the dz tile is the
//     A operand, the activated input halo the B operand, k = four pixel rows of one column.  It writes its own partial tile, and
//     folds its fp32 accumulators into that tile every D_WG_CHUNK items once a range is longer than that (large N);
//     k_disc_wgrad_reduce sums the partials (fp64, fixed order) into [Cout, Cin, 3, 3].  The workgroups of channel block 0 also sum
//     dz per channel: the bias gradient.
//   * k_disc_dgrad<CD, CX, S, HEAD>: data gradient of layers 8, 5, 2 in gather form: a workgroup owns a tile of INPUT pixels (for
//     stride 2 of one parity class (iy % 2, ix % 2), whose taps are a fixed subset) and all CX channels, so no two workgroups write
//     one element.  Contraction over 8-channel chunks of dz; weights are read from the forward's packed blob, transposed in staging.
//   * k_disc_wgrad0 / k_disc_wgrad0_reduce / k_disc_dgrad0: layer 0 (K = 27) on the VALU; LeakyReLU's mask is a0 > 0.
//   * k_disc_masks: testing aid, the four masks as the kernels above decide them.
//   * k_disc_pack: a discriminator's packed blob from its convolutions' parameter tensors, on the device (this one's ten, or the
//     SRGAN discriminator's fourteen).
// The SRGAN trainer's discriminator (cid_srd_backward, srgan_disc_bwd_kernels.h) runs its layers 0-10 on these kernels as they are
// and its 128 -> 256 layer on further instantiations, through trailing template arguments that default to the kernels above: POOL, the
// upstream gradient in a third form (D_UP_POOL: one value per image and channel, what an average pool passes down); CD_PART, the
// data gradient reading the packed weights in COUT-channel parts; CD_TOTAL, the weight gradient running one part per grid z.
#pragma once
#include "disc_kernels.h"

namespace cid {

constexpr int D_COEF = 8;

// Where the gradient of a BatchNorm's activated output comes from: a tensor; the denoise head's rank-one dl[n] * coef[c][7]; or
// one value per (image, channel), up[n][c] (the pooled head of the SRGAN discriminator: dm[n][c] / P).
constexpr int D_UP_TENSOR = 0, D_UP_HEAD = 1, D_UP_POOL = 2;

__device__ __forceinline__ float d_slope(float y) { return y > 0.0f ? 1.0f : 0.2f; }

// dz of one element from its raw z, the upstream gradient and the channel's coef.
__device__ __forceinline__ float d_bn_dz(const float* cf, float z, float up) {
    const float g = up * d_slope(d_bn(cf[0], z, cf[1]));
    return cf[2] * (g - cf[5] - (z - cf[3]) * cf[4] * cf[6]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// Head.  Same thread layout and summation order as k_disc_head.
struct DiscHeadBwdArgs {
    const float* z;          // z8
    const float* st;         // BN9 (scale, shift)
    const float* w;          // 1x1 weights [128], then the bias
    const float* grad_prob;  // [N]
    double* mean;            // out [N][128]: mean over pixels of a8
    float* dl;               // out [N]: gradient of the logit
    long long P;
    int n0;
};

__global__ void __launch_bounds__(D_HEAD_THREADS) k_disc_head_bwd(const DiscHeadBwdArgs a) {
    __shared__ double red[D_HEAD_THREADS];
    const int tid = threadIdx.x, c = tid & 127, grp = tid >> 7;
    const size_t n = (size_t)a.n0 + blockIdx.x;
    const float s = a.st[2 * c], sh = a.st[2 * c + 1];
    const float* zc = a.z + ((n * 16 + c / 8) * (size_t)a.P) * 8 + (c & 7);
    double sum = 0.0;
    for (long long p = grp; p < a.P; p += D_HEAD_GROUPS) sum += (double)d_lrelu(d_bn(s, zc[p * 8], sh));
    red[tid] = sum;
    __syncthreads();
    double tot = 0.0;
    if (tid < 128) {
        for (int g = 0; g < D_HEAD_GROUPS; ++g) tot += red[g * 128 + tid];
        tot /= (double)a.P;
        a.mean[n * 128 + tid] = tot;
        tot *= (double)a.w[tid];
    }
    __syncthreads();
    if (tid < 128) red[tid] = tot;
    __syncthreads();
    for (int off = 64; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const double logit = (double)a.w[128] + red[0];
        const double p = 1.0 / (1.0 + exp(-logit));
        a.dl[n] = (float)((double)a.grad_prob[n] * p * (1.0 - p));
    }
}

struct DiscHeadReduceArgs {
    const double* mean;
    const float* dl;
    const float* w;      // 1x1 weights [128]
    float* dw;           // out [128], may be null
    float* db;           // out [1], may be null
    float* coef;         // BN9 coef: slot 7 <- w12[c] / P
    double P;
    int N;
};

__global__ void __launch_bounds__(128) k_disc_head_reduce(const DiscHeadReduceArgs a) {
    const int c = threadIdx.x;
    a.coef[c * D_COEF + 7] = (float)((double)a.w[c] / a.P);
    if (a.dw) {
        double s = 0.0;
        for (int n = 0; n < a.N; ++n) s += (double)a.dl[n] * a.mean[(size_t)n * 128 + c];
        a.dw[c] = (float)s;
    }
    if (a.db && c == 0) {
        double s = 0.0;
        for (int n = 0; n < a.N; ++n) s += (double)a.dl[n];
        a.db[0] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// BatchNorm backward, the two per-channel sums.  A workgroup owns one image's strip of D_BN_STRIP pixels and all C channels: thread
// = (channel block, pixel slot, half of the block); the pixel slots of a channel are added in a fixed order.
constexpr int D_BN_STRIP = 512;

struct DiscBnPartArgs {
    const float* z;       // raw z of this BatchNorm, C8
    const float* up;      // gradient of the activated tensor, C8 (unused with HEAD)
    const float* dl;      // HEAD: [N]; POOL: [N][C]
    const float* coef;    // HEAD: slot 7 of this layer's coef
    const float* st;      // (scale, shift) pairs
    const double* mi;     // (mean, invstd) pairs
    double* slab;         // slab[(c*2 + k)*rows + row], k = 0: sum g, 1: sum g*xh; row = image * strips + strip
    long long rows, P;
    int strips, n0;
};

template <int C, bool HEAD, bool POOL = false>
__global__ void __launch_bounds__(D_THREADS) k_disc_bn_bwd_part(const DiscBnPartArgs a) {
    static_assert(!(HEAD && POOL), "one form of upstream gradient");
    constexpr int UP = POOL ? D_UP_POOL : (HEAD ? D_UP_HEAD : D_UP_TENSOR);
    constexpr int PS = D_THREADS / (C / 4);   // pixel slots
    __shared__ double red[D_THREADS * 8];
    const int tid = threadIdx.x, half = tid & 1, ps = (tid >> 1) % PS, cb = tid / (2 * PS);
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const long long p0 = (long long)blockIdx.x * D_BN_STRIP;
    const long long p1 = p0 + D_BN_STRIP < a.P ? p0 + D_BN_STRIP : a.P;
    const size_t base = ((n * (C / 8) + cb) * (size_t)a.P) * 8 + half * 4;
    float s[4], t[4], mean[4], inv[4], uh[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = cb * 8 + half * 4 + j;
        s[j] = a.st[2 * c];
        t[j] = a.st[2 * c + 1];
        mean[j] = (float)a.mi[2 * c];
        inv[j] = (float)a.mi[2 * c + 1];
        uh[j] = HEAD ? a.dl[n] * a.coef[c * D_COEF + 7] : (UP == D_UP_POOL ? a.dl[n * C + c] : 0.0f);
    }
    double acc[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long p = p0 + ps; p < p1; p += PS) {
        const d_f32x4 z = *reinterpret_cast<const d_f32x4*>(a.z + base + (size_t)p * 8);
        d_f32x4 u = d_f32x4{uh[0], uh[1], uh[2], uh[3]};
        if (UP == D_UP_TENSOR) u = *reinterpret_cast<const d_f32x4*>(a.up + base + (size_t)p * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float g = u[j] * d_slope(d_bn(s[j], z[j], t[j]));
            const float xh = (z[j] - mean[j]) * inv[j];
            acc[2 * j] += (double)g;
            acc[2 * j + 1] += (double)g * (double)xh;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[tid * 8 + i] = acc[i];
    __syncthreads();
    if (tid < C) {
        const int cb2 = tid >> 3, h2 = (tid & 7) >> 2, j = tid & 3;
        double r0 = 0.0, r1 = 0.0;
        for (int q = 0; q < PS; ++q) {
            const int src = ((cb2 * PS + q) * 2 + h2) * 8 + 2 * j;
            r0 += red[src];
            r1 += red[src + 1];
        }
        const long long row = (long long)n * a.strips + blockIdx.x;
        a.slab[(size_t)(tid * 2) * a.rows + row] = r0;
        a.slab[(size_t)(tid * 2 + 1) * a.rows + row] = r1;
    }
}

struct DiscBnRedArgs {
    const double* slab;
    long long rows;
    double count;          // N * Hl * Wl
    const float* gamma;
    const float* st;
    const double* mi;
    int training;
    float* coef;           // out: slots 0..6 of this layer
    float* dgamma;         // out [C], may be null
    float* dbeta;          // out [C], may be null
};

__global__ void __launch_bounds__(D_THREADS) k_disc_bn_bwd_reduce(const DiscBnRedArgs a) {
    __shared__ double r1[D_THREADS], r2[D_THREADS];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double* p1 = a.slab + (size_t)(c * 2) * a.rows;
    const double* p2 = p1 + a.rows;
    double s1 = 0.0, s2 = 0.0;
    for (long long i = tid; i < a.rows; i += D_THREADS) {
        s1 += p1[i];
        s2 += p2[i];
    }
    r1[tid] = s1;
    r2[tid] = s2;
    __syncthreads();
    for (int off = D_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            r1[tid] += r1[tid + off];
            r2[tid] += r2[tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double dbeta = r1[0], dgamma = r2[0];
        const double mean = a.mi[2 * c], inv = a.mi[2 * c + 1];
        float* cf = a.coef + c * D_COEF;
        cf[0] = a.st[2 * c];
        cf[1] = a.st[2 * c + 1];
        cf[2] = (float)((double)a.gamma[c] * inv);
        cf[3] = (float)mean;
        cf[4] = (float)inv;
        cf[5] = a.training ? (float)(dbeta / a.count) : 0.0f;
        cf[6] = a.training ? (float)(dgamma / a.count) : 0.0f;
        if (a.dgamma) a.dgamma[c] = (float)dgamma;
        if (a.dbeta) a.dbeta[c] = (float)dbeta;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Operand shared by wgrad and dgrad: where dz comes from.
struct DiscDzSrc {
    const float* z;      // C8, CD channels, Ho x Wo: the saved raw z of this convolution
    const float* up;     // C8, same shape: gradient of the activated tensor (null with HEAD)
    const float* dl;     // HEAD: [N]; POOL: [N][all channels of the tensor]
    const float* coef;   // [CD][D_COEF]
};

// Four consecutive channels (first channel c of lds_cf, a multiple of 4) of dz at element offset `off` of image n.  POOL: `pool` is
// the index of lds_cf's channel 0 of this image in dl.
template <int UP>
__device__ __forceinline__ d_f32x4 d_load_dz(const DiscDzSrc& s, const float* lds_cf, size_t n, size_t off, int c, size_t pool = 0) {
    const d_f32x4 z = *reinterpret_cast<const d_f32x4*>(s.z + off);
    d_f32x4 u;
    if (UP == D_UP_HEAD) {
        const float dl = s.dl[n];
#pragma unroll
        for (int j = 0; j < 4; ++j) u[j] = dl * lds_cf[(c + j) * D_COEF + 7];
    } else if (UP == D_UP_POOL) {
        u = *reinterpret_cast<const d_f32x4*>(s.dl + pool + c);
    } else {
        u = *reinterpret_cast<const d_f32x4*>(s.up + off);
    }
    d_f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = d_bn_dz(lds_cf + (c + j) * D_COEF, z[j], u[j]);
    return r;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Data gradient of a 3x3 convolution, stride S, pad 1: out[n, ci, iy, ix] = sum_{co, kh, kw} dz[n, co, oy, ox] * W[co, ci, kh, kw]
// with iy = S*oy + kh - 1.  In class coordinates (iy = S*i + py, ix = S*j + px) the taps of a class read dz at (i + d, j + e) with
// d, e in {-1, 0, 1} for S = 1 and in {0, 1} for S = 2 (py = 0: kh = 1, d = 0;  py = 1: kh = 0, d = 1 and kh = 2, d = 0), so the
// B operand is a stride-1 read of a dz halo whatever S is.
struct DiscDgradArgs {
    DiscDzSrc dz;
    const float* w;       // the forward's packed weights of this layer: [CX/8][9 taps][8][CD] (CD_PART < CD: one such block of
                          // CD_PART channels, then their biases, per part: DiscConvArgs::w)
    float* out;           // C8, CX channels, Hin x Win
    int Hin, Win, Ho, Wo;
    int tiles_x;          // tiles per tile row of class (0, 0), the largest class
    int n0;
};

template <int CD, int CX, int S>
struct DiscDgradGeom {
    static constexpr int WN = CX / 64;
    static constexpr int WM = 4 / WN;
    static constexpr int TH = 4 * WM;                            // class rows per tile
    static constexpr int HOFF = S == 1 ? 1 : 0;                  // halo rows / columns before the tile
    static constexpr int HH = TH + (S == 1 ? 2 : 1);
    static constexpr int HWD = D_TW + (S == 1 ? 2 : 1);
    static constexpr int NPIX = HH * HWD;
    static constexpr int XSTR = NPIX + ((16 - NPIX % 32) + 32) % 32;   // 16 mod 32: planes k and k+1 on disjoint banks (DiscGeom, S = 1)
    static constexpr int WSTR = CX + 16;
    static constexpr int CHUNKS = CD / 8;
    static constexpr int STAGE_ITERS = (NPIX * 2 + D_THREADS - 1) / D_THREADS;
    static constexpr int CLASSES = S * S;
    static_assert(CX == 64 || CX == 128, "64 channels per wave");
    static_assert(S == 1 || S == 2, "stride");
};

// POOL: the upstream gradient is D_UP_POOL (HEAD false).  CD_PART < CD: the packed weights come in CD_PART-channel parts.  Left at
// their defaults the kernel is the denoise discriminator's.
template <int CD, int CX, int S, bool HEAD, bool POOL = false, int CD_PART = CD>
__global__ void __launch_bounds__(D_THREADS, 2) k_disc_dgrad(const DiscDgradArgs a) {
    static_assert(CD % CD_PART == 0 && !(HEAD && POOL), "whole parts, one form of upstream gradient");
    constexpr int UP = POOL ? D_UP_POOL : (HEAD ? D_UP_HEAD : D_UP_TENSOR);
    using G = DiscDgradGeom<CD, CX, S>;
    constexpr int WM = G::WM, TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR, HOFF = G::HOFF;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];
    __shared__ float lds_cf[CD * D_COEF];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l16 = lane & 15, kq = lane >> 4;
    const int cls = blockIdx.z, py = S == 2 ? cls >> 1 : 0, px = S == 2 ? cls & 1 : 0;
    const int Hc = (a.Hin - py + S - 1) / S, Wc = (a.Win - px + S - 1) / S;   // rows / columns of this class
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int i0 = ty * TH, j0 = tx * D_TW;
    if (i0 >= Hc || j0 >= Wc) return;   // the whole workgroup: a smaller class has fewer tiles
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const size_t out_plane = (size_t)a.Ho * a.Wo;
    const int ny = S == 1 ? 3 : 1 + py, nx = S == 1 ? 3 : 1 + px;

    for (int i = tid; i < CD * D_COEF; i += D_THREADS) lds_cf[i] = a.dz.coef[i];

    d_f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * 4) * HWD + l16;
    const int wb = kq * WSTR + wn * 64 + l16;

    for (int chunk = 0; chunk < G::CHUNKS; ++chunk) {
        __syncthreads();
        // ---- dz halo of this chunk: global (z, upstream) -> dz -> LDS planes
        const size_t src = ((n * (CD / 8) + chunk) * out_plane) * 8;
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int oy = i0 - HOFF + hy, ox = j0 - HOFF + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (oy >= 0 && oy < a.Ho && ox >= 0 && ox < a.Wo)
                    v = d_load_dz<UP>(a.dz, lds_cf, n, src + ((size_t)oy * a.Wo + ox) * 8 + h * 4, chunk * 8 + h * 4, n * CD);
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights, transposed: row (tap, dz channel) holds the CX input channels
        for (int i = tid; i < 18 * CX; i += D_THREADS) {
            const int ci = i % CX, r = i / CX, h = r & 1, tap = r >> 1;
            const size_t row = (size_t)((ci >> 3) * 9 + tap) * 8 + (ci & 7);
            d_f32x4 v;
            if constexpr (CD_PART == CD) {
                v = *reinterpret_cast<const d_f32x4*>(a.w + row * CD + chunk * 8 + h * 4);
            } else {   // the chunk's part of the weights, and its channels there
                const int wpart = chunk * 8 / CD_PART;
                const float* wp = a.w + (size_t)wpart * (CX * 9 * CD_PART + CD_PART);
                v = *reinterpret_cast<const d_f32x4*>(wp + row * CD_PART + (chunk * 8 - wpart * CD_PART) + h * 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_w[(tap * 8 + h * 4 + j) * WSTR + ci] = v[j];
        }
        __syncthreads();
        for (int ay = 0; ay < ny; ++ay) {
            const int kh = S == 1 ? ay : (py ? 2 * ay : 1);
            const int dy = S == 1 ? 2 - ay : (py ? 1 - ay : 0);    // halo row of the tile's row 0 for this tap
            for (int ax = 0; ax < nx; ++ax) {
                const int kw = S == 1 ? ax : (px ? 2 * ax : 1);
                const int dx = S == 1 ? 2 - ax : (px ? 1 - ax : 0);
                const int tap = kh * 3 + kw;
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    float av[4], bv[4];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct) av[ct] = lds_w[wb + (tap * 8 + sub * 4) * WSTR + ct * 16];
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) bv[pt] = lds_x[xb + sub * 4 * XSTR + (pt + dy) * HWD + dx];
#pragma unroll
                    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
                }
            }
        }
    }

    const int j = j0 + l16;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const int i = i0 + wm * 4 + pt;
        if (i < Hc && j < Wc) {
            const int iy = i * S + py, ix = j * S + px;
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int ci = wn * 64 + ct * 16 + kq * 4;
                *reinterpret_cast<d_f32x4*>(a.out + (((n * (CX / 8) + ci / 8) * a.Hin + iy) * (size_t)a.Win + ix) * 8 + (ci & 7)) = acc[ct][pt];
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Weight gradient of a 3x3 convolution, stride S, pad 1: dW[co, ci, kh, kw] = sum_{n, oy, ox} dz[n, co, oy, ox] * a[n, ci, S*oy+kh-1, S*ox+kw-1].
struct DiscWgradArgs {
    DiscDzSrc dz;
    const float* ain;      // C8, CX channels, Hin x Win: a0, or the previous convolution's raw z (BN_IN)
    const float* st_in;    // BN_IN: (scale, shift) of the previous BatchNorm
    float* part;           // out: part[(((split*(CX/16) + block)*CD + co)*9 + tap)*16 + ci%16]   (CD: all channels of the layer)
    double* part_b;        // out: part_b[split*CD + co] (written by channel block 0)
    long long items;       // N * tiles
    int splits;
    int Hin, Win, Ho, Wo;
    int tiles_x, tiles;
};

constexpr int D_WG_TH = 4;   // output rows per item: the four k of one MFMA
// A workgroup's range of items grows with N (items / splits), and one fp32 chain over all of it drifts: 2.4e-5 of max|dW| over the
// 1640 items a workgroup gets at N = 35000 of 24 x 40, against 2e-6 up to about a hundred.  Past D_WG_CHUNK items the accumulators
// are folded into the workgroup's own partial tile in memory every D_WG_CHUNK items (each lane adds to the words it wrote itself),
// so that both chains stay short and no register is spent on it; a range of at most D_WG_CHUNK items never folds and keeps the
// bits it always had.
constexpr int D_WG_CHUNK = 64;

template <int S>
struct DiscWgradGeom {
    static constexpr int HH = (D_WG_TH - 1) * S + 3;
    static constexpr int HWD = (D_TW - 1) * S + 3;
    // B operand read: lanes 0-15 are 16 channel planes, lanes 16-31 the same planes one k (S halo rows) further.  S = 1: plane
    // stride 2 mod 32 and an odd row stride; S = 2: plane stride 1 mod 32 and a row stride of 8 mod 16.  Conflict-free either way.
    static constexpr int RS = S == 1 ? HWD + 1 : HWD + 7;
    static constexpr int NP = HH * RS;
    static constexpr int XSTR = NP + (((S == 1 ? 2 : 1) - NP % 32) + 32) % 32;
    static constexpr int ZSTR = D_WG_TH * D_TW + 1;   // A operand: channel stride 1 mod 32, k stride 16
    static_assert(S == 1 ? (RS % 2 == 1) : (RS % 16 == 8), "row stride");
};

// POOL: the upstream gradient is D_UP_POOL (HEAD false).  CD_TOTAL > CD: the layer has CD_TOTAL dz channels and the grid's z counts
// its CD-channel parts (as k_disc_conv's COUT_TOTAL): grid = (splits, CX / 16, CD_TOTAL / CD).
template <int CD, int CX, int S, bool BN_IN, bool HEAD, bool POOL = false, int CD_TOTAL = CD>
__global__ void __launch_bounds__(D_THREADS, 2) k_disc_wgrad(const DiscWgradArgs a) {
    static_assert(CD_TOTAL % CD == 0 && !(HEAD && POOL), "whole parts, one form of upstream gradient");
    constexpr int UP = POOL ? D_UP_POOL : (HEAD ? D_UP_HEAD : D_UP_TENSOR);
    using G = DiscWgradGeom<S>;
    constexpr int HH = G::HH, HWD = G::HWD, RS = G::RS, XSTR = G::XSTR, ZSTR = G::ZSTR;
    constexpr int RT = CD / 64;   // 16-channel row tiles per wave
    __shared__ float lds_a[16 * XSTR];
    __shared__ float lds_z[CD * ZSTR];
    __shared__ float lds_cf[CD * D_COEF];
    __shared__ float lds_st[BN_IN ? 32 : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x, blk = blockIdx.y;
    const long long it0 = a.items * split / a.splits, it1 = a.items * (split + 1) / a.splits;
    const size_t in_plane = (size_t)a.Hin * a.Win, out_plane = (size_t)a.Ho * a.Wo;
    const int co0 = CD_TOTAL == CD ? 0 : (int)blockIdx.z * CD;   // first dz channel of this part

    for (int i = tid; i < CD * D_COEF; i += D_THREADS) lds_cf[i] = a.dz.coef[co0 * D_COEF + i];
    if (BN_IN && tid < 32) lds_st[tid] = a.st_in[blk * 32 + tid];

    d_f32x4 acc[RT][9];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) acc[r][tap] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const bool fold = it1 - it0 > D_WG_CHUNK;
    double bsum = 0.0;

    // a lane holds dz channels 4*kq .. 4*kq+3 of its row tile for input channel l16
    float* part = a.part + (((size_t)split * (CX / 16) + blk) * CD_TOTAL + co0) * 144;
    auto store_acc = [&](bool add) {
        float* dst = part;
        asm volatile("" : "+v"(dst));   // the addresses are formed here, not kept in registers across the item loop
#pragma unroll
        for (int r = 0; r < RT; ++r)
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float* o = dst + ((size_t)((wave * RT + r) * 16 + kq * 4 + e) * 9 + tap) * 16 + l16;
                    *o = add ? *o + acc[r][tap][e] : acc[r][tap][e];
                }
                if (add) asm volatile("" ::: "memory");   // four loads in flight, not all 36 RT: a fold costs no registers
            }
    };

    const int zb = ((wave * RT) * 16 + l16) * ZSTR + kq * D_TW;
    const int ab = l16 * XSTR + kq * S * RS;

    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.tiles);
        const int t = (int)(item - (long long)n * a.tiles), ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const int oy0 = ty * D_WG_TH, ox0 = tx * D_TW;
        const int iy0 = oy0 * S - 1, ix0 = ox0 * S - 1;
        __syncthreads();   // every wave is done with the previous item (and lds_cf, lds_st are visible before the first one)
        // ---- dz tile: CD channels x 4 x 16 pixels (0 outside the tensor)
        for (int idx = tid; idx < CD * 16; idx += D_THREADS) {
            const int h = idx & 1, c = (idx >> 1) & 15, r = (idx >> 5) & 3, cb = idx >> 7;
            const int oy = oy0 + r, ox = ox0 + c;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (oy < a.Ho && ox < a.Wo)
                v = d_load_dz<UP>(a.dz, lds_cf, n, ((n * (CD_TOTAL / 8) + co0 / 8 + cb) * out_plane + (size_t)oy * a.Wo + ox) * 8 + h * 4,
                                  cb * 8 + h * 4, n * CD_TOTAL + co0);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_z[(cb * 8 + h * 4 + j) * ZSTR + r * D_TW + c] = v[j];
        }
        // ---- halo of the 16 input channels of this block (BatchNorm + LeakyReLU of the previous layer; 0 outside the image)
        for (int idx = tid; idx < HH * HWD * 4; idx += D_THREADS) {
            const int q = idx / (HH * HWD), p = idx - q * (HH * HWD), cb2 = q >> 1, h = q & 1;
            const int hy = p / HWD, hx = p - hy * HWD;
            const int iy = iy0 + hy, ix = ix0 + hx;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) {
                v = *reinterpret_cast<const d_f32x4*>(a.ain + ((n * (CX / 8) + blk * 2 + cb2) * in_plane + (size_t)iy * a.Win + ix) * 8 + h * 4);
                if (BN_IN) {
                    const int c = cb2 * 8 + h * 4;
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = d_lrelu(d_bn(lds_st[2 * (c + j)], v[j], lds_st[2 * (c + j) + 1]));
                }
            }
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
                const float bv = lds_a[ab + (tap / 3) * RS + col * S + tap % 3];
#pragma unroll
                for (int r = 0; r < RT; ++r) acc[r][tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[r], bv, acc[r][tap], 0, 0, 0);
            }
        }
        if (fold && (item - it0 + 1) % D_WG_CHUNK == 0) {
            store_acc(item - it0 + 1 > D_WG_CHUNK);   // the first fold writes: the workspace may hold anything
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int tap = 0; tap < 9; ++tap) acc[r][tap] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        }
    }
    store_acc(fold);
    if (blk == 0 && tid < CD) a.part_b[(size_t)split * CD_TOTAL + co0 + tid] = bsum;
}

struct DiscWgradReduceArgs {
    const float* part;
    const double* part_b;
    float* dw;      // out [CD][CX][3][3], may be null
    float* db;      // out [CD], may be null
    int splits, CD, CX;
};

__global__ void __launch_bounds__(D_THREADS) k_disc_wgrad_reduce(const DiscWgradReduceArgs a) {
    const int o = blockIdx.x * D_THREADS + threadIdx.x;
    const int nw = a.CD * a.CX * 9;
    if (o < nw) {
        if (!a.dw) return;
        const int tap = o % 9, ci = (o / 9) % a.CX, co = o / (9 * a.CX);
        const size_t stride = (size_t)(a.CX / 16) * a.CD * 144;
        const float* p = a.part + (((size_t)(ci >> 4) * a.CD + co) * 9 + tap) * 16 + (ci & 15);
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += (double)p[k * stride];
        a.dw[o] = (float)s;
    } else if (o < nw + a.CD) {
        if (!a.db) return;
        const int co = o - nw;
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += a.part_b[(size_t)k * a.CD + co];
        a.db[co] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Layer 0.  dz0 = da0 * (a0 > 0 ? 1 : 0.2).
__device__ __forceinline__ d_f32x4 d_dz0(const float* a0, const float* da0, size_t off) {
    const d_f32x4 y = *reinterpret_cast<const d_f32x4*>(a0 + off);
    d_f32x4 g = *reinterpret_cast<const d_f32x4*>(da0 + off);
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] *= d_slope(y[j]);
    return g;
}

// Weight and bias gradient: dW0[co, k] = sum_{n, p} dz0[n, co, p] * patch[n, p, k], k = (ci*3 + kh)*3 + kw, and k = 27 the constant 1
// (the bias).  A workgroup walks a contiguous range of (image, 64-pixel strip) items; thread = (channel co, group of 7 k).
struct DiscWgrad0Args {
    const void* in;        // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    const float* a0;
    const float* da0;
    double* part;          // out: part[(split*64 + co)*28 + k]
    long long items;       // N * strips
    int splits, strips;
    int H, W;
};

template <bool U8>
__global__ void __launch_bounds__(D_THREADS) k_disc_wgrad0(const DiscWgrad0Args a) {
    __shared__ float lds_d[64 * 64];   // [pixel][co]
    __shared__ float lds_p[64 * 28];   // [pixel][k]
    const int tid = threadIdx.x, co = tid & 63, kg = tid >> 6;
    const long long HW = (long long)a.H * a.W;
    const long long it0 = a.items * blockIdx.x / a.splits, it1 = a.items * (blockIdx.x + 1) / a.splits;
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.strips);
        const long long p0 = (item - (long long)n * a.strips) * 64;
        __syncthreads();
        for (int idx = tid; idx < 64 * 16; idx += D_THREADS) {
            const int h = idx & 1, px = (idx >> 1) & 63, cb = idx >> 7;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (p0 + px < HW) v = d_dz0(a.a0, a.da0, ((n * 8 + cb) * (size_t)HW + (size_t)(p0 + px)) * 8 + h * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_d[px * 64 + cb * 8 + h * 4 + j] = v[j];
        }
        for (int idx = tid; idx < 64 * 28; idx += D_THREADS) {
            const int px = idx / 28, k = idx - px * 28;
            const long long p = p0 + px;
            float v = 0.0f;
            if (p < HW) {
                if (k == 27) {
                    v = 1.0f;
                } else {
                    const int ci = k / 9, kh = (k / 3) % 3, kw = k % 3;
                    const int y = (int)(p / a.W), x = (int)(p - (long long)y * a.W);
                    const int iy = y + kh - 1, ix = x + kw - 1;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                        const size_t pix = (size_t)iy * a.W + ix;
                        if (U8) v = d_u8(static_cast<const unsigned char*>(a.in)[(n * HW + pix) * 3 + ci]);
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

struct DiscWgrad0ReduceArgs {
    const double* part;
    float* dw;     // out [64][27], may be null
    float* db;     // out [64], may be null
    int splits;
};

__global__ void __launch_bounds__(D_THREADS) k_disc_wgrad0_reduce(const DiscWgrad0ReduceArgs a) {
    const int o = blockIdx.x * D_THREADS + threadIdx.x;
    if (o >= 64 * 28) return;
    const int co = o / 28, k = o - co * 28;
    float* dst = k == 27 ? (a.db ? a.db + co : nullptr) : (a.dw ? a.dw + co * 27 + k : nullptr);
    if (!dst) return;
    double s = 0.0;
    for (int i = 0; i < a.splits; ++i) s += a.part[(size_t)i * 64 * 28 + o];
    *dst = (float)s;
}

// Input gradient: dx[n, ci, y, x] = sum_{co, kh, kw} dz0[n, co, y+1-kh, x+1-kw] * W0[co, ci, kh, kw].  One thread per pixel.
struct DiscDgrad0Args {
    const float* a0;
    const float* da0;
    const float* w;     // [64][3][3][3]
    float* out;         // fp32 [N,3,H,W]
    int H, W;
    int n0;
};

__global__ void __launch_bounds__(D_THREADS) k_disc_dgrad0(const DiscDgrad0Args a) {
    const int p = blockIdx.x * D_THREADS + threadIdx.x;
    const long long HW = (long long)a.H * a.W;
    if (p >= HW) return;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int y = p / a.W, x = p - y * a.W;
    typedef __attribute__((address_space(4))) const float* ConstF;
    const ConstF wc = (ConstF)a.w;
    float acc[3] = {0.0f, 0.0f, 0.0f};
    for (int kh = 0; kh < 3; ++kh) {
        const int oy = y + 1 - kh;
        if (oy < 0 || oy >= a.H) continue;
        for (int kw = 0; kw < 3; ++kw) {
            const int ox = x + 1 - kw;
            if (ox < 0 || ox >= a.W) continue;
            const size_t pix = (size_t)oy * a.W + ox;
            for (int cb = 0; cb < 8; ++cb) {
                const size_t off = ((n * 8 + cb) * (size_t)HW + pix) * 8;
                const d_f32x4 d0 = d_dz0(a.a0, a.da0, off), d1 = d_dz0(a.a0, a.da0, off + 4);
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float d = j < 4 ? d0[j & 3] : d1[j & 3];
                    const int wbase = (cb * 8 + j) * 27 + kh * 3 + kw;
#pragma unroll
                    for (int ci = 0; ci < 3; ++ci) acc[ci] = fmaf(wc[wbase + ci * 9], d, acc[ci]);
                }
            }
        }
    }
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) a.out[(n * 3 + ci) * HW + p] = acc[ci];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Testing aid: LeakyReLU's mask of one layer as the kernels above decide it, uint8 [N, C, P] (1 where the slope is 1).
struct DiscMaskArgs {
    const float* z;       // C8: a0 (st null) or a raw z
    const float* st;      // (scale, shift) pairs, or null: mask = z > 0
    unsigned char* out;
    long long total;      // N * C * P
    long long P;
    int C;
};

__global__ void __launch_bounds__(D_THREADS) k_disc_masks(const DiscMaskArgs a) {
    const long long o = (long long)blockIdx.x * D_THREADS + threadIdx.x;
    if (o >= a.total) return;
    const long long p = o % a.P, nc = o / a.P;
    const int c = (int)(nc % a.C);
    const long long n = nc / a.C;
    const float z = a.z[((n * (a.C / 8) + c / 8) * a.P + p) * 8 + (c & 7)];
    const float y = a.st ? d_bn(a.st[2 * c], z, a.st[2 * c + 1]) : z;
    a.out[o] = d_slope(y) == 1.0f ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------------------
// A discriminator's packed blob from its convolutions' parameter tensors (reference layouts, device memory): what cid_disc_set_weight
// + cid_disc_upload_weights, or the SRGAN discriminator's pair, build on the host, byte for byte (alignment gaps are 0).  part[l] > 0:
// layer l is packed [CIN/8][9 taps][8][part] with its part biases behind, one such block per part output channels (pack_mfma_layer,
// api_common.h); part[l] = 0: it keeps the reference layout, weights then biases.
constexpr int D_PACK_LAYERS = 7;

struct DiscPackArgs {
    const float* w[D_PACK_LAYERS];
    const float* b[D_PACK_LAYERS];
    float* blob;
    int off[D_PACK_LAYERS], cin[D_PACK_LAYERS], cout[D_PACK_LAYERS], kk[D_PACK_LAYERS], part[D_PACK_LAYERS];
    int layers;   // slots in use
    int total;
};

__global__ void __launch_bounds__(D_THREADS) k_disc_pack(const DiscPackArgs a) {
    const int i = blockIdx.x * D_THREADS + threadIdx.x;
    if (i >= a.total) return;
    int off = a.off[0], cout = a.cout[0], cin = a.cin[0], kk = a.kk[0], part = a.part[0];
    const float* w = a.w[0];
    const float* b = a.b[0];
#pragma unroll
    for (int k = 1; k < D_PACK_LAYERS; ++k)
        if (k < a.layers && i >= a.off[k]) {
            off = a.off[k];
            cout = a.cout[k];
            cin = a.cin[k];
            kk = a.kk[k];
            part = a.part[k];
            w = a.w[k];
            b = a.b[k];
        }
    const int r = i - off, nw = cout * cin * kk;
    float v = 0.0f;
    if (part > 0) {
        const int nwp = cin * 9 * part, block = nwp + part;
        const int pi = r / block, rr = r - pi * block;
        if (pi < cout / part) {
            if (rr < nwp) {
                const int co = pi * part + rr % part, q = rr / part, ci8 = q & 7, tap = (q >> 3) % 9, chunk = (q >> 3) / 9;
                v = w[((size_t)co * cin + chunk * 8 + ci8) * 9 + tap];
            } else {
                v = b[pi * part + rr - nwp];
            }
        }
    } else if (r < nw) {
        v = w[r];
    } else if (r < nw + cout) {
        v = b[r - nw];
    }
    a.blob[i] = v;
}

}  // namespace cid
