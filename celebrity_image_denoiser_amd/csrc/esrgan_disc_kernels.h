// esrgan_disc_kernels.h — gfx950 device kernels of the ESRGAN trainer's discriminator forward (cid_esd_forward, include/cid.h),
// reference backend/trainingcode/esrgan_code/models.py:36-71: four 3x3 stride-2 convolutions 3 -> 64 -> 128 -> 256 -> 512, each
// followed by LeakyReLU(0.2), then view(N, -1) and Linear(512 * H4 * W4, 1).  No BatchNorm, no sigmoid: the output is the logit.
//
// Activations are fp32 in the C8 layout of disc_kernels.h.  Every kernel stores the ACTIVATED tensor (LeakyReLU in the epilogue), so
// the next layer's halo padding is plain zero and a backward pass recovers the LeakyReLU mask as a > 0.
//   * k_esd_conv1<U8>: conv1 + bias + LeakyReLU on the VALU, one thread per OUTPUT pixel (K = 27 is too short for the matrix cores),
//     the 27 inputs of the pixel in registers, the weights wave-uniform through scalar loads, as k_disc_conv0.  It reads fp32
//     [N,3,H,W] or uint8 [N,H,W,3] decoded as ToTensor() does, (float)u / 255.0f: the expression of the ESRGAN generator's head
//     (esrgan_kernels.h), so a uint8 batch and its fp32 copy give identical bits.
//   * k_esd_conv<CIN, COUT_TOTAL, PT>: conv2, conv3, conv4 as an implicit GEMM on v_mfma_f32_16x16x4_f32 (exact fp32), in the operand
//     arrangement of k_disc_conv<., 64, 2>: weights are the A operand (MFMA rows = output channels), 16 consecutive output pixels of
//     one row the B operand, so a lane's four accumulators are four consecutive channels of one pixel and leave as one 16-byte store.
//     A 256-thread workgroup owns a tile of (4 * PT) x 16 output pixels and ONE 64-channel part of the COUT_TOTAL channels (grid z =
//     part); wave w owns the PT rows w * PT ... w * PT + PT - 1 of the tile (4 * PT accumulator tiles).  PT = 4, 2, 1 for conv2, conv3,
//     conv4 halves the tile's rows each time the image halves, which keeps the workgroup count of the three launches equal (DESIGN
//     section 25).  The contraction runs over 8-channel input chunks (32 of them at CIN = 256): the chunk's halo is staged global ->
//     VGPR -> LDS planes (positions outside the image as 0), the chunk's 72 x 64 weights next to it.  Each output element is one
//     accumulation chain in the order (chunk, tap, channel), whatever PT, N or the image's place in the batch.
//   * k_esd_fc: the flatten and Linear(512 * H4 * W4, 1), one 1024-thread workgroup per image.  fc.weight is permuted into C8 order
//     when it is packed, so the dot product reads two contiguous streams with 16-byte loads; products and sums are fp64, each thread
//     over quads t, t + 1024, ... and the 1024 partial sums by a tree: an order that depends on H4 * W4 alone.
//   * k_esd_losses: the trainer's three BCE-with-logits means (esrgan_train.py:104-119) in fp64 in a fixed order;
//     k_esd_trainer_losses adds the pixel MSE and the two sums the trainer forms of them.
// No atomics.  Offsets are 64-bit; only a pixel index inside one image is an int.
#pragma once
#include "disc_kernels.h"

namespace cid {

// ---------------------------------------------------------------------------------------------------------------------------
// conv1: Conv2d(3, 64, 3, stride=2, padding=1) + bias + LeakyReLU(0.2) -> a1 (C8 layout, 64 channels, Ho x Wo).
struct EsdConv1Args {
    const void* in;     // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    float* out;         // a1
    const float* w;     // [64][3][3][3] reference order, then the 64 biases
    int H, W, Ho, Wo;
    int n0;             // first image of this launch (grid y = image - n0)
};

template <bool U8>
__global__ void __launch_bounds__(D_THREADS) k_esd_conv1(const EsdConv1Args a) {
    const int p = blockIdx.x * D_THREADS + threadIdx.x;
    const int HWo = a.Ho * a.Wo;
    if (p >= HWo) return;
    const size_t HW = (size_t)a.H * a.W;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int y = p / a.Wo, x = p - y * a.Wo;
    float xin[27];
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int kh = 0; kh < 3; ++kh)
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = 2 * y + kh - 1, ix = 2 * x + kw - 1;
                float v = 0.0f;
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const size_t pix = (size_t)iy * a.W + ix;
                    if (U8) v = (float)static_cast<const unsigned char*>(a.in)[(n * HW + pix) * 3 + ci] / 255.0f;
                    else v = static_cast<const float*>(a.in)[(n * 3 + ci) * HW + pix];
                }
                xin[(ci * 3 + kh) * 3 + kw] = v;
            }
    // constant address space: uniform addresses become scalar loads (k_disc_conv0)
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
        d_f32x4* o = reinterpret_cast<d_f32x4*>(a.out + ((n * 8 + cb) * (size_t)HWo + p) * 8);
        o[0] = d_f32x4{v[0], v[1], v[2], v[3]};
        o[1] = d_f32x4{v[4], v[5], v[6], v[7]};
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// conv2, conv3, conv4: 3x3 convolution, stride 2, padding 1, + bias + LeakyReLU, as an implicit GEMM on v_mfma_f32_16x16x4_f32.
constexpr int ESD_PART = 64;   // output channels per workgroup

struct EsdConvArgs {
    const float* in;      // C8, CIN channels, Hin x Win, activated
    float* out;           // C8, COUT_TOTAL channels, Ho x Wo, activated
    const float* w;       // per 64-channel part: [CIN/8][9 taps][8][64] (w[((chunk*9 + tap)*8 + ci%8)*64 + co%64]), then its 64 biases
    int Hin, Win, Ho, Wo;
    int tiles_x;          // tiles per tile row
    int n0;
};

template <int CIN, int PT>
struct EsdGeom {
    static constexpr int TH = 4 * PT;                           // output rows per tile (four waves of PT rows)
    static constexpr int HH = (TH - 1) * 2 + 3;                 // halo rows
    static constexpr int HWD = (D_TW - 1) * 2 + 3;              // halo columns
    static constexpr int NPIX = HH * HWD;
    // LDS plane stride of the halo: lanes 0-15 of a B-operand read are on 16 pixels two apart in plane k, lanes 16-31 on the same
    // pixels of plane k + 1; with an odd stride the two sets fall on banks of opposite parity (DiscGeom, S = 2).
    static constexpr int XSTR = NPIX + ((1 - NPIX % 32) + 32) % 32;
    static constexpr int WSTR = ESD_PART + 16;                  // weight row stride in LDS: rows k and k + 1 on disjoint banks
    static constexpr int CHUNKS = CIN / 8;
    static constexpr int STAGE_ITERS = (NPIX * 2 + D_THREADS - 1) / D_THREADS;
    static_assert(PT == 1 || PT == 2 || PT == 4, "rows per wave");
    static_assert(CIN % 8 == 0, "8-channel chunks");
    static_assert(XSTR % 2 == 1, "odd plane stride");
};

template <int CIN, int COUT_TOTAL, int PT>
__global__ void __launch_bounds__(D_THREADS, 2) k_esd_conv(const EsdConvArgs a) {
    static_assert(COUT_TOTAL % ESD_PART == 0, "whole parts");
    using G = EsdGeom<CIN, PT>;
    constexpr int TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];

    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int iy0 = ty * TH * 2 - 1, ix0 = tx * D_TW * 2 - 1;
    const size_t in_plane = (size_t)a.Hin * a.Win;
    const int co0 = (int)blockIdx.z * ESD_PART;                                        // first channel of this part
    const float* wpart = a.w + (size_t)blockIdx.z * (CIN * 9 * ESD_PART + ESD_PART);   // its weights and biases

    d_f32x4 acc[4][PT];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * PT * 2) * HWD + l16 * 2;   // this lane's B operand base (plane kq, its pixel column)
    const int wb = kq * WSTR + l16;                             // this lane's A operand base (row kq, its channel)

    for (int chunk = 0; chunk < G::CHUNKS; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk
        // ---- halo of this chunk: global -> VGPR -> LDS planes
        const float* src = a.in + ((n * (CIN / 8) + chunk) * in_plane) * 8;
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int iy = iy0 + hy, ix = ix0 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};   // outside the image: the zero padding of the activated tensor
                if (iy >= 0 && iy < a.Hin && ix >= 0 && ix < a.Win)
                    v = *reinterpret_cast<const d_f32x4*>(src + ((size_t)iy * a.Win + ix) * 8 + h * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights: 72 rows (tap, channel) of 64
        const float* wsrc = wpart + (size_t)chunk * 72 * ESD_PART;
        for (int i = tid; i < 72 * ESD_PART / 4; i += D_THREADS) {
            const int r = i / (ESD_PART / 4), c4 = i - r * (ESD_PART / 4);
            *reinterpret_cast<d_f32x4*>(&lds_w[r * WSTR + c4 * 4]) = *reinterpret_cast<const d_f32x4*>(wsrc + (size_t)r * ESD_PART + c4 * 4);
        }
        __syncthreads();
        // ---- 9 taps x 2 k-steps of 4 channels: 4 * PT MFMAs per k-step per wave
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int kh = tap / 3, kw = tap % 3;
#pragma unroll
            for (int sub = 0; sub < 2; ++sub) {
                float av[4], bv[PT];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) av[ct] = lds_w[wb + (tap * 8 + sub * 4) * WSTR + ct * 16];
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) bv[pt] = lds_x[xb + sub * 4 * XSTR + (pt * 2 + kh) * HWD + kw];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: + bias, LeakyReLU, store (four consecutive channels of one pixel per lane)
    const float* bias = wpart + (size_t)CIN * 9 * ESD_PART;
    const int ox = tx * D_TW + l16;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int co = ct * 16 + kq * 4;   // first of this lane's four channels within the part
        const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(bias + co);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            const int oy = ty * TH + wm * PT + pt;
            if (oy < a.Ho && ox < a.Wo) {
                const d_f32x4 z = acc[ct][pt] + b4;
                *reinterpret_cast<d_f32x4*>(a.out + (((n * (COUT_TOTAL / 8) + (co0 + co) / 8) * a.Ho + oy) * (size_t)a.Wo + ox) * 8 + (co & 7)) =
                    d_f32x4{d_lrelu(z[0]), d_lrelu(z[1]), d_lrelu(z[2]), d_lrelu(z[3])};
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// fc: view(N, -1) + Linear(512 * P, 1), P = H4 * W4.  One workgroup per image.  In C8 order an image's a4 is F = 512 * P consecutive
// floats and the packed fc.weight has the same order, so thread t multiplies the quads t, t + 1024, ... of both streams.
constexpr int ESD_FC_THREADS = D_LOSS_THREADS;
struct EsdFcArgs {
    const float* a4;    // C8, 512 channels, P pixels per image
    const float* w;     // fc.weight in C8 order [64][P][8], then (64-float aligned) the bias
    const float* bias;
    float* out;         // logits [N]
    long long F;        // 512 * P
    int n0;
};

__global__ void __launch_bounds__(ESD_FC_THREADS) k_esd_fc(const EsdFcArgs a) {
    __shared__ double red[ESD_FC_THREADS];
    const size_t n = (size_t)a.n0 + blockIdx.x;
    const d_f32x4* x = reinterpret_cast<const d_f32x4*>(a.a4 + n * (size_t)a.F);
    const d_f32x4* w = reinterpret_cast<const d_f32x4*>(a.w);
    const long long quads = a.F / 4;
    double sum = 0.0;
    for (long long q = threadIdx.x; q < quads; q += ESD_FC_THREADS) {
        const d_f32x4 xv = x[q], wv = w[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) sum += (double)xv[j] * (double)wv[j];
    }
    sum = d_block_sum(sum, red);
    if (threadIdx.x == 0) a.out[n] = (float)(sum + (double)a.bias[0]);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The ESRGAN trainer's losses of one batch (esrgan_train.py:104-119): one workgroup, fp64, fixed order.
// One image pair's three BCE-with-logits terms in the stable form max(x, 0) - x*y + log1p(exp(-|x|)): real against 1, fake against 0,
// fake against 1, each added to its running sum.  The one statement of the term.
__device__ __forceinline__ void e_bce_terms(double xr, double xf, double& real1, double& fake0, double& fake1) {
    const double sr = log1p(exp(-fabs(xr))), sf = log1p(exp(-fabs(xf)));
    real1 += fmax(xr, 0.0) - xr + sr;
    fake0 += fmax(xf, 0.0) + sf;
    fake1 += fmax(xf, 0.0) - xf + sf;
}

struct EsdLossArgs {
    const float* x_real;   // logits D(clean) [N]
    const float* x_fake;   // logits D(denoised) [N]
    int N;
    double* out;
};

// The three means over the batch (every thread gets them).
__device__ __forceinline__ void e_bce_means(const EsdLossArgs& a, double* red, double& real1, double& fake0, double& fake1) {
    real1 = fake0 = fake1 = 0.0;
    for (int i = threadIdx.x; i < a.N; i += D_LOSS_THREADS) e_bce_terms(a.x_real[i], a.x_fake[i], real1, fake0, fake1);
    real1 = d_block_sum(real1, red) / a.N;
    fake0 = d_block_sum(fake0, red) / a.N;
    fake1 = d_block_sum(fake1, red) / a.N;
}

//   out[0] mean BCE(real, 1)    out[1] mean BCE(fake, 0)    out[2] mean BCE(fake, 1)
__global__ void __launch_bounds__(D_LOSS_THREADS) k_esd_losses(const EsdLossArgs a) {
    __shared__ double red[D_LOSS_THREADS];
    double real1, fake0, fake1;
    e_bce_means(a, red, real1, fake0, fake1);
    if (threadIdx.x == 0) {
        a.out[0] = real1;
        a.out[1] = fake0;
        a.out[2] = fake1;
    }
}

// An image operand of the pixel loss: fp32 [N,3,H,W], or uint8 [N,H,W,3] decoded as conv1 decodes it, visited in [N,3,H,W] order.
__device__ __forceinline__ float e_img(const void* p, int fmt, long long i, long long HW) {
    if (fmt == 1) {
        const long long n = i / (3 * HW), r = i - n * 3 * HW, c = r / HW, pix = r - c * HW;
        return (float)static_cast<const unsigned char*>(p)[(n * HW + pix) * 3 + c] / 255.0f;
    }
    return static_cast<const float*>(p)[i];
}

struct EsdTrainerLossArgs {
    EsdLossArgs bce;
    const void* den;
    const void* clean;
    int fd, fc;           // 0 = fp32 NCHW, 1 = uint8 NHWC
    long long HW;
};

//   out[0] d_loss = 0.5 * (BCE(real, 1) + BCE(fake, 0))    out[1] gan_loss = BCE(fake, 1)
//   out[2] pixel_loss = MSE(denoised, clean)               out[3] g_loss = pixel_loss + 1e-3 * gan_loss
// The MSE is the reduction of k_disc_losses: thread t over elements t, t + 1024, ... in fp64, then d_block_sum.  g_loss is a rounded
// product and a rounded sum (no fused multiply-add), so it equals the same expression on the two stored values.
__global__ void __launch_bounds__(D_LOSS_THREADS) k_esd_trainer_losses(const EsdTrainerLossArgs a) {
    __shared__ double red[D_LOSS_THREADS];
    const long long count = (long long)a.bce.N * 3 * a.HW;
    double se = 0.0;
    for (long long i = threadIdx.x; i < count; i += D_LOSS_THREADS) {
        const float d = e_img(a.den, a.fd, i, a.HW) - e_img(a.clean, a.fc, i, a.HW);
        se += (double)d * (double)d;
    }
    se = d_block_sum(se, red);
    double real1, fake0, fake1;
    e_bce_means(a.bce, red, real1, fake0, fake1);
    if (threadIdx.x == 0) {
        const double pixel = se / (double)count;
        a.bce.out[0] = 0.5 * (real1 + fake0);
        a.bce.out[1] = fake1;
        a.bce.out[2] = pixel;
        a.bce.out[3] = __dadd_rn(pixel, __dmul_rn(1e-3, fake1));
    }
}

}  // namespace cid
