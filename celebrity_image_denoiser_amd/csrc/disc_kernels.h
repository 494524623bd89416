// disc_kernels.h — gfx950 device kernels of the trainer's DenoiseDiscriminator forward (cid_disc_forward, include/cid.h),
// reference backend/trainingcode/denoise_gan_code/training.py:77-98.
//
// Activations between launches are fp32 in a channel-blocked layout ("C8"): element (n, c, y, x) of a C-channel H x W tensor is at
//     (((n * (C/8) + c/8) * H + y) * W + x) * 8 + c % 8,
// so the eight channels of one input chunk of a halo row are one contiguous run of memory.
//   * k_disc_conv0: layer 0 (Conv2d(3, 64, 3, p=1) + bias + LeakyReLU) on the VALU, one thread per pixel (K = 27 is too short for the
//     matrix cores); it writes the activated a0.
//   * k_disc_conv<CIN, COUT, S, BN_IN, STATS>: layers 2, 5, 8 (3x3 convolution, stride S, pad 1) as an implicit GEMM on
//     v_mfma_f32_16x16x4_f32 (exact fp32).  Weights are the A operand (MFMA rows = output channels), pixels the B operand (columns =
//     16 consecutive output pixels of one row), so a lane's four accumulators are four consecutive channels of one pixel and leave as
//     one 16-byte store.  A 256-thread workgroup owns a tile of (4 * WAVES_M) x 16 output pixels and all COUT channels; each wave
//     owns 4 rows x 16 pixels x 64 channels (16 accumulator tiles).  The contraction runs over 8-channel input chunks: the chunk's
//     halo is staged global -> VGPR -> LDS, and with BN_IN the PREVIOUS layer's BatchNorm and LeakyReLU, max-form
//     y = s*z + t, y > 0 ? y : 0.2*y, is applied once per staged element there.  Halo positions outside the image are written as 0:
//     the reference pads the activated tensor, so padding is zero AFTER BatchNorm and LeakyReLU.  The kernel stores the raw
//     pre-BatchNorm z = conv + bias.  With STATS (train mode) every workgroup also writes its per-channel sums of z and z^2, in fp64,
//     to its own row of a slab (no atomics).  A sixth template argument COUT_TOTAL > COUT runs a wider layer as COUT_TOTAL / COUT
//     channel parts, one per grid z (the SRGAN discriminator's 128 -> 256 layer, srgan_disc_kernels.h); left at its default it is COUT
//     and the kernel is the single-part one.
//   * k_disc_bn_stats (train): one workgroup per channel reduces the slab in a fixed order in fp64, writes the channel's (scale,
//     shift) for the next layer's staging and updates running_mean / running_var in the module's own buffers.
//   * k_disc_bn_eval (eval): (scale, shift) of all of a discriminator's BatchNorms from the running buffers, one workgroup each (three
//     here, four in the SRGAN discriminator).
//     Both also write the (mean, invstd) pairs in fp64 when the call keeps its tensors for a backward pass (cid_disc_forward_saved;
//     the backward kernels are in disc_bwd_kernels.h).
//   * k_disc_head: one 1024-thread workgroup per image: BN9 + LeakyReLU of z8, the global average (fp64, fixed order), the 1x1 convolution and
//     the sigmoid.
//   * k_disc_bn_count (train): num_batches_tracked += 1 of those BatchNorms, after every statistics launch has read them.
//   * k_disc_losses: the trainer's BCE / MSE reductions over one batch (fp64, fixed order).
// An image's tiles depend only on (H, W), never on N or on its position in the batch.
#pragma once
#include <hip/hip_runtime.h>

namespace cid {

constexpr int D_THREADS = 256;
constexpr int D_TW = 16;   // output pixels per tile row (one MFMA column tile)

typedef float d_f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float d_lrelu(float v) { return v > 0.0f ? v : v * 0.2f; }

// BatchNorm as the kernels apply it: y = s*z + t in one fused multiply-add.  Every forward kernel and every backward kernel
// (disc_bwd_kernels.h) evaluates y through this function, so the backward's LeakyReLU mask (y > 0) is the forward's decision.
__device__ __forceinline__ float d_bn(float s, float z, float t) { return fmaf(s, z, t); }

// u8 image -> fp32 as ToTensor + Normalize(0.5, 0.5) with true divisions: the forward's u8 input arithmetic (k_conv_head).
__device__ __forceinline__ float d_u8(unsigned char u) { return ((float)u / 255.0f - 0.5f) / 0.5f; }

// ---------------------------------------------------------------------------------------------------------------------------
// Layer 0: Conv2d(3, 64, 3, padding=1) + bias + LeakyReLU(0.2) -> a0 (C8 layout, 64 channels).
struct DiscConv0Args {
    const void* in;     // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    float* out;         // a0
    const float* w;     // [64][3][3][3] reference order, then the 64 biases
    int H, W;
    int n0;             // first image of this launch (grid y = image - n0)
};

template <bool U8>
__global__ void __launch_bounds__(D_THREADS) k_disc_conv0(const DiscConv0Args a) {
    const int p = blockIdx.x * D_THREADS + threadIdx.x;
    const long long HW = (long long)a.H * a.W;
    if (p >= HW) return;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int y = p / a.W, x = p - y * a.W;
    float xin[27];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = y + kh - 1, ix = x + kw - 1;
                float v = 0.0f;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const size_t pix = (size_t)iy * a.W + ix;
                    if (U8) v = d_u8(static_cast<const unsigned char*>(a.in)[(n * HW + pix) * 3 + ci]);
                    else v = static_cast<const float*>(a.in)[(n * 3 + ci) * HW + pix];
                }
                xin[(ci * 3 + kh) * 3 + kw] = v;
            }
    // The weights are read through the constant address space: uniform addresses there become scalar loads (through a generic
    // pointer the compiler cannot rule out that the output stores clobber them and issues a vector load per weight).
    typedef __attribute__((address_space(4))) const float* ConstF;
    const ConstF wc = (ConstF)a.w;
    const ConstF bias = wc + 64 * 27;
    for (int cb = 0; cb < 8; ++cb) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = cb * 8 + j;
            float acc = bias[c];
#pragma unroll
            for (int k = 0; k < 27; ++k) acc = fmaf(wc[c * 27 + k], xin[k], acc);
            v[j] = d_lrelu(acc);
        }
        d_f32x4* o = reinterpret_cast<d_f32x4*>(a.out + ((n * 8 + cb) * HW + p) * 8);
        o[0] = d_f32x4{v[0], v[1], v[2], v[3]};
        o[1] = d_f32x4{v[4], v[5], v[6], v[7]};
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Layers 2, 5, 8: 3x3 convolution, stride S, padding 1, as an implicit GEMM on v_mfma_f32_16x16x4_f32.
struct DiscConvArgs {
    const float* in;      // C8, CIN channels, Hin x Win (a0, or the previous layer's raw z)
    float* out;           // C8, COUT channels, Ho x Wo: z = conv + bias (before BatchNorm)
    const float* w;       // packed: [CIN/8][9 taps][8][COUT] (w[((chunk*9 + tap)*8 + ci%8)*COUT + co]), then the COUT biases;
                          // with COUT_TOTAL > COUT one such block (weights, then biases) per COUT-channel part, back to back
    const float* st_in;   // BN_IN: (scale, shift) of the previous BatchNorm, float pairs [CIN]
    double* slab;         // STATS: slab[(co*2 + k)*rows + row], k = 0: sum z, 1: sum z^2; row = image * tiles + tile
    long long rows;
    int Hin, Win, Ho, Wo;
    int tiles_x, tiles;   // tiles per tile row / per image
    int n0;
};

template <int CIN, int COUT, int S>
struct DiscGeom {
    static constexpr int WN = COUT / 64;                        // waves across channels
    static constexpr int WM = 4 / WN;                           // waves across pixel rows
    static constexpr int TH = 4 * WM;                           // output rows per tile
    static constexpr int HH = (TH - 1) * S + 3;                 // halo rows
    static constexpr int HWD = (D_TW - 1) * S + 3;              // halo columns
    static constexpr int NPIX = HH * HWD;
    // LDS plane stride of the halo (one plane per chunk channel).  A B-operand read has lanes 0-15 on 16 pixels S apart in plane
    // k and lanes 16-31 on the same pixels in plane k+1; ds_read_b32 banks are (dword mod 32) per half-wave, so the stride is
    // 16 mod 32 for S = 1 and odd for S = 2: conflict-free either way.
    static constexpr int XSTR = S == 1 ? NPIX + ((16 - NPIX % 32) + 32) % 32 : NPIX + ((1 - NPIX % 32) + 32) % 32;
    static constexpr int WSTR = COUT + 16;                      // weight row stride in LDS: rows k and k+1 on disjoint banks
    static constexpr int CHUNKS = CIN / 8;
    static constexpr int STAGE_ITERS = (NPIX * 2 + D_THREADS - 1) / D_THREADS;
    static_assert(COUT == 64 || COUT == 128, "64 channels per wave");
    static_assert(CIN % 8 == 0, "8-channel chunks");
};

// COUT_TOTAL > COUT: the tensor has COUT_TOTAL channels and the launch's grid z counts its COUT-channel parts; workgroup z computes
// channels z*COUT ... z*COUT + COUT - 1 from part z of the weights (DiscConvArgs::w), staging the input halo itself.
template <int CIN, int COUT, int S, bool BN_IN, bool STATS, int COUT_TOTAL = COUT>
__global__ void __launch_bounds__(D_THREADS, 2) k_disc_conv(const DiscConvArgs a) {
    static_assert(COUT_TOTAL % COUT == 0, "whole parts");
    using G = DiscGeom<CIN, COUT, S>;
    constexpr int WM = G::WM, TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];
    __shared__ float lds_st[BN_IN ? 2 * CIN : 1];
    __shared__ double lds_red[STATS ? WM * COUT * 2 : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int iy0 = ty * TH * S - 1, ix0 = tx * D_TW * S - 1;
    const size_t in_plane = (size_t)a.Hin * a.Win;
    const int co0 = COUT_TOTAL == COUT ? 0 : (int)blockIdx.z * COUT;                                       // first channel of this part
    const float* wpart = COUT_TOTAL == COUT ? a.w : a.w + (size_t)blockIdx.z * (CIN * 9 * COUT + COUT);   // its weights and biases

    if (BN_IN)
        for (int i = tid; i < 2 * CIN; i += D_THREADS) lds_st[i] = a.st_in[i];

    d_f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * 4 * S) * HWD + l16 * S;   // this lane's B operand base (plane kq, its pixel column)
    const int wb = kq * WSTR + wn * 64 + l16;                  // this lane's A operand base (row kq, its channel)

    for (int chunk = 0; chunk < G::CHUNKS; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk (and lds_st is visible before the first one)
        // ---- halo of this chunk: global -> VGPR -> (BatchNorm + LeakyReLU of the previous layer) -> LDS planes
        const float* src = a.in + ((n * (CIN / 8) + chunk) * in_plane) * 8;
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int iy = iy0 + hy, ix = ix0 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};   // outside the image: the zero padding of the activated tensor
                if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win) {
                    v = *reinterpret_cast<const d_f32x4*>(src + ((size_t)iy * a.Win + ix) * 8 + h * 4);
                    if (BN_IN) {
                        const int c = chunk * 8 + h * 4;
#pragma unroll
                        for (int j = 0; j < 4; ++j) v[j] = d_lrelu(d_bn(lds_st[2 * (c + j)], v[j], lds_st[2 * (c + j) + 1]));
                    }
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights: 72 rows (tap, channel) of COUT
        const float* wsrc = wpart + (size_t)chunk * 72 * COUT;
        for (int i = tid; i < 72 * COUT / 4; i += D_THREADS) {
            const int r = i / (COUT / 4), c4 = i - r * (COUT / 4);
            *reinterpret_cast<d_f32x4*>(&lds_w[r * WSTR + c4 * 4]) = *reinterpret_cast<const d_f32x4*>(wsrc + (size_t)r * COUT + c4 * 4);
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
                for (int pt = 0; pt < 4; ++pt) bv[pt] = lds_x[xb + sub * 4 * XSTR + (pt * S + kh) * HWD + kw];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: + bias, store z (four consecutive channels of one pixel per lane), per-channel partial sums
    const float* bias = wpart + (size_t)CIN * 9 * COUT;
    const int ox = tx * D_TW + l16;
    bool ok[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) ok[pt] = (ty * TH + wm * 4 + pt) < a.Ho && ox < a.Wo;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int co = wn * 64 + ct * 16 + kq * 4;   // first of this lane's four channels
        const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(bias + co);
        double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const d_f32x4 z = acc[ct][pt] + b4;
            if (ok[pt]) {
                const int oy = ty * TH + wm * 4 + pt;
                *reinterpret_cast<d_f32x4*>(a.out + (((n * (COUT_TOTAL / 8) + (co0 + co) / 8) * a.Ho + oy) * (size_t)a.Wo + ox) * 8 + (co & 7)) = z;
                if (STATS)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const double d = (double)z[r];
                        s1[r] += d;
                        s2[r] += d * d;
                    }
            }
        }
        if (STATS) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) {
                    s1[r] += __shfl_xor(s1[r], off, 64);
                    s2[r] += __shfl_xor(s2[r], off, 64);
                }
                if (l16 == 0) {
                    lds_red[(wm * COUT + co + r) * 2] = s1[r];
                    lds_red[(wm * COUT + co + r) * 2 + 1] = s2[r];
                }
            }
        }
    }
    if (STATS) {
        __syncthreads();
        if (tid < COUT) {
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                t1 += lds_red[(m * COUT + tid) * 2];
                t2 += lds_red[(m * COUT + tid) * 2 + 1];
            }
            const long long row = (long long)n * a.tiles + t;
            a.slab[(size_t)((co0 + tid) * 2) * a.rows + row] = t1;
            a.slab[(size_t)((co0 + tid) * 2 + 1) * a.rows + row] = t2;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Train-mode BatchNorm statistics of one layer: grid = channels.
struct DiscStatsArgs {
    const double* slab;
    long long rows;
    double count;                 // N * Ho * Wo values per channel
    const float* gamma;
    const float* beta;
    float* running_mean;
    float* running_var;
    const long long* num_batches_tracked;
    double eps, momentum;         // momentum < 0: None (1 / num_batches_tracked after this call's increment)
    float* st;                    // out: (scale, shift) pairs [C]
    double* mi;                   // out, may be null: (mean, invstd) pairs [C] that the backward pass normalises with
};

__global__ void __launch_bounds__(D_THREADS) k_disc_bn_stats(const DiscStatsArgs a) {
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
        const double M = a.count;
        const double mean = r1[0] / M;
        double var = r2[0] / M - mean * mean;   // biased: what the normalisation uses
        if (var < 0.0) var = 0.0;
        const double var_u = var * (M / (M - 1.0));   // unbiased: what running_var tracks
        const double sc = (double)a.gamma[c] / sqrt(var + a.eps);
        a.st[2 * c] = (float)sc;
        a.st[2 * c + 1] = (float)((double)a.beta[c] - mean * sc);
        if (a.mi) {
            a.mi[2 * c] = mean;
            a.mi[2 * c + 1] = 1.0 / sqrt(var + a.eps);
        }
        const double m = a.momentum < 0.0 ? 1.0 / (double)(a.num_batches_tracked[0] + 1) : a.momentum;
        a.running_mean[c] = (float)((1.0 - m) * (double)a.running_mean[c] + m * mean);
        a.running_var[c] = (float)((1.0 - m) * (double)a.running_var[c] + m * var_u);
    }
}

// Eval-mode (scale, shift) of a discriminator's BatchNorms from their running buffers: grid = its BatchNorms (up to D_MAX_BNS),
// block = D_BN_MAXC channels.
constexpr int D_MAX_BNS = 4;
constexpr int D_BN_MAXC = 256;

struct DiscBnEvalArgs {
    const float* gamma[D_MAX_BNS];
    const float* beta[D_MAX_BNS];
    const float* running_mean[D_MAX_BNS];
    const float* running_var[D_MAX_BNS];
    double eps[D_MAX_BNS];
    float* st[D_MAX_BNS];
    int C[D_MAX_BNS];
    double* mi[D_MAX_BNS];        // may be null: (running_mean, invstd) pairs [C] for the backward pass
};

// Channel c of one eval-mode BatchNorm: its (scale, shift) and, where `mi` is not null, its (running_mean, invstd).
__device__ __forceinline__ void d_bn_eval_channel(const float* gamma, const float* beta, const float* running_mean,
                                                  const float* running_var, double eps, float* st, double* mi, int c) {
    const double sc = (double)gamma[c] / sqrt((double)running_var[c] + eps);
    st[2 * c] = (float)sc;
    st[2 * c + 1] = (float)((double)beta[c] - (double)running_mean[c] * sc);
    if (mi) {
        mi[2 * c] = (double)running_mean[c];
        mi[2 * c + 1] = 1.0 / sqrt((double)running_var[c] + eps);
    }
}

__global__ void __launch_bounds__(D_BN_MAXC) k_disc_bn_eval(const DiscBnEvalArgs a) {
    const int l = blockIdx.x, c = threadIdx.x;
    if (c >= a.C[l]) return;
    d_bn_eval_channel(a.gamma[l], a.beta[l], a.running_mean[l], a.running_var[l], a.eps[l], a.st[l], a.mi[l], c);
}

struct DiscBnCountArgs {
    long long* count[D_MAX_BNS];
    int n;
};

__global__ void __launch_bounds__(64) k_disc_bn_count(const DiscBnCountArgs a) {
    if ((int)threadIdx.x < a.n) a.count[threadIdx.x][0] += 1;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Head: BatchNorm9 + LeakyReLU of z8, AdaptiveAvgPool2d(1), Conv2d(128, 1, 1), Sigmoid.  One 1024-thread workgroup per image:
// channel = thread % 128, pixel group = thread / 128 (pixels g, g + 8, ...); the eight group sums are added in a fixed order.
constexpr int D_HEAD_THREADS = 1024;
constexpr int D_HEAD_GROUPS = D_HEAD_THREADS / 128;
struct DiscHeadArgs {
    const float* z;     // z8, C8, 128 channels, P = H4 * W4 pixels per image
    const float* st;    // BN9 (scale, shift) pairs [128]
    const float* w;     // 1x1 weights [128], then the bias
    float* out;         // [N]
    long long P;
    int n0;
};

__global__ void __launch_bounds__(D_HEAD_THREADS) k_disc_head(const DiscHeadArgs a) {
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
        tot = (double)a.w[tid] * (tot / (double)a.P);
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
        a.out[n] = (float)(1.0 / (1.0 + exp(-logit)));
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The trainer's losses of one batch (training.py:412-424): one workgroup, fp64, fixed order.
//   out[0] d_loss = BCE(p_real, 1) + BCE(p_fake, 0)    out[1] g_loss = content + 0.001 * adv
//   out[2] content_loss = MSE(denoised, clean)         out[3] adv_loss = BCE(p_fake, 1)
// BCE clamps its logs at -100 like nn.BCELoss.  Image operands are fp32 [N,3,H,W] or uint8 [N,H,W,3] (decoded as the forward does);
// the MSE visits the elements in [N,3,H,W] order whatever the format.
constexpr int D_LOSS_THREADS = 1024;

struct DiscLossArgs {
    const float* p_real;
    const float* p_fake;
    const void* den;
    const void* clean;
    int fd, fc;           // 0 = fp32 NCHW, 1 = uint8 NHWC
    int N;
    long long HW;
    double* out;
};

__device__ __forceinline__ float d_img(const void* p, int fmt, long long i, long long HW) {
    if (fmt == 1) {
        const long long n = i / (3 * HW), r = i - n * 3 * HW, c = r / HW, pix = r - c * HW;
        return d_u8(static_cast<const unsigned char*>(p)[(n * HW + pix) * 3 + c]);
    }
    return static_cast<const float*>(p)[i];
}

__device__ __forceinline__ double d_block_sum(double v, double* red) {
    const int tid = threadIdx.x;
    red[tid] = v;
    __syncthreads();
    for (int off = D_LOSS_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// One image's three BCE terms, logs clamped at -100: -log(p_real) (target 1), -log(1 - p_fake) (target 0), -log(p_fake) (target 1),
// each added to its running sum.  The one statement of the term: k_disc_losses and k_srd_losses (srgan_disc_kernels.h) call it.
__device__ __forceinline__ void d_bce_terms(double pr, double pf, double& real1, double& fake0, double& fake1) {
    real1 -= fmax(log(pr), -100.0);
    fake0 -= fmax(log(1.0 - pf), -100.0);
    fake1 -= fmax(log(pf), -100.0);
}

__global__ void __launch_bounds__(D_LOSS_THREADS) k_disc_losses(const DiscLossArgs a) {
    __shared__ double red[D_LOSS_THREADS];
    const int tid = threadIdx.x;
    const long long count = (long long)a.N * 3 * a.HW;
    double se = 0.0;
    for (long long i = tid; i < count; i += D_LOSS_THREADS) {
        const float d = d_img(a.den, a.fd, i, a.HW) - d_img(a.clean, a.fc, i, a.HW);
        se += (double)d * (double)d;
    }
    double real1 = 0.0, fake0 = 0.0, fake1 = 0.0;
    for (int i = tid; i < a.N; i += D_LOSS_THREADS) d_bce_terms(a.p_real[i], a.p_fake[i], real1, fake0, fake1);
    se = d_block_sum(se, red);
    real1 = d_block_sum(real1, red);
    fake0 = d_block_sum(fake0, red);
    fake1 = d_block_sum(fake1, red);
    if (tid == 0) {
        const double content = se / (double)count, adv = fake1 / a.N;
        a.out[0] = real1 / a.N + fake0 / a.N;
        a.out[1] = content + 0.001 * adv;
        a.out[2] = content;
        a.out[3] = adv;
    }
}

}  // namespace cid
