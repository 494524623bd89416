// vgg_kernels.h — gfx950 device kernels of torchvision VGG16 `features` as LPIPS(net='vgg') and the trainers' VGGPerceptualLoss use it
// (cid_vgg_lpips, cid_vgg_content_loss; the definition is in the header comment of include/cid.h).
//
// Both towers run as ONE batch of 2 N images, fp32 in the C8 layout of disc_kernels.h, as in lpips_kernels.h.
//   * k_vgg_head: operand read (fp32 [N,3,H,W] as it is, uint8 [N,H,W,3] through d_u8), the optional v*0.5+0.5, the optional scaling
//     layer, Conv2d(3,64,3,pad 1), bias and ReLU on the VALU (K = 27).  A one-wave workgroup owns 64 consecutive pixels of the batch's
//     pixel sequence (q = n * H * W + pixel, in grid.x) and all 64 channels; the weight rows are wave-uniform scalar loads, a
//     pixel's sum is one chain in (ci, kh, kw) order plus the bias.
//   * The other twelve convolutions are k_lpips_conv<CIN, COUT, 3, POOL, 2, XPOS> (lpips_kernels.h): the batch-as-one-column-sequence
//     implicit GEMM on v_mfma_f32_16x16x4_f32 with, under POOL, the 2x2 / stride-2 floor-mode maximum taken while the operand is
//     staged.  A 128-column run of a map wider than 339 can stage more than LP_XPOS positions per plane (vg_stage_bound); such
//     launches take planes of VG_XPOS_WIDE positions (65 KB of LDS with the weights: still two workgroups per CU) and serve maps
//     up to VG_MAX_SIDE wide.
//   * k_lpips_dist<VgTaps>: the distance kernel over taps of 64, 128, 256, 512, 512 channels.
//   * k_vgg_content: one workgroup per image pair: the mean of (f_a - f_b)^2 over relu3_3, in double, a fixed-order tree.
// Nothing is atomic; offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include "lpips_kernels.h"

namespace cid {

constexpr int VG_CONVS = 13;
constexpr int VG_MAX_SIDE = 512;       // the largest accepted H or W
constexpr int VG_XPOS_WIDE = 3328;     // = 0 mod 64 and mod D_THREADS

// Positions a workgroup of a 3x3 launch stages per plane, at most.  lp_stage_bound counts 2 halo rows per touched image and whole
// rows for a run of LP_NT columns wherever it starts; for a map of at least LP_NT pixels that is up to twice what can happen.  Such
// a run touches at most two images; the part in the first ends with that image's last row, the part in the second starts with its
// first row, so L1 + L2 = LP_NT columns lie in at most ceil(L1 / Wo) + ceil(L2 / Wo) <= LP_NT / Wo + 2 rows, plus 2 halo rows per
// image.  A run inside one image touches no more rows than that.
__host__ __device__ constexpr long long vg_stage_bound(int Ho, int Wo) {
    return (long long)Ho * Wo >= LP_NT ? (long long)(LP_NT / Wo + 6) * (Wo + 2) : lp_stage_bound(Ho, Wo, 1);
}
static_assert(vg_stage_bound(VG_MAX_SIDE, VG_MAX_SIDE) <= VG_XPOS_WIDE && vg_stage_bound(1, VG_MAX_SIDE) <= VG_XPOS_WIDE, "the widest map's run fits a wide plane");

struct VgTaps {
    static __host__ __device__ constexpr int channels(int k) { return k == 0 ? 64 : k == 1 ? 128 : k == 2 ? 256 : 512; }
    static __host__ __device__ constexpr int lin_off(int k) { return k == 0 ? 0 : k == 1 ? 64 : k == 2 ? 192 : k == 3 ? 448 : 960; }
};
constexpr int VG_LIN_SEG = 1472;

// ---------------------------------------------------------------------------------------------------------------------------
// Head.  Segment: w[k][64] with k = (ci * 3 + kh) * 3 + kw, bias[64], shift[3] at VG_HEAD_SS, scale[3] at VG_HEAD_SS + 4.
constexpr int VG_HEAD_K = 27;
constexpr int VG_HEAD_B = VG_HEAD_K * 64, VG_HEAD_SS = VG_HEAD_B + 64, VG_HEAD_SEG = VG_HEAD_SS + 64;
constexpr int VG_HEAD_PIX = 64;   // pixels of the batch sequence per workgroup (one wave)

struct VgHeadArgs {
    const void* a;      // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    const void* b;
    float* out;         // relu1_1: C8, 64 channels, H x W, 2 N images
    const float* w;     // the head's segment
    long long total;    // 2 N * H * W pixels
    int H, W;
    int N;              // images per tower
    int u8a, u8b;       // operand formats
    int unit;           // v * 0.5 + 0.5 first
    int scaled;         // the scaling layer (x - shift) / scale
};

__global__ void __launch_bounds__(VG_HEAD_PIX) k_vgg_head(const VgHeadArgs a) {
    const int lane = threadIdx.x;
    const long long q = (long long)blockIdx.x * VG_HEAD_PIX + lane;
    const bool valid = q < a.total;
    const long long qq = valid ? q : 0;
    const size_t HW = (size_t)a.H * a.W;
    const size_t n = (size_t)(qq / (long long)HW);
    const int p = (int)(qq - (long long)(n * HW));
    const int oy = p / a.W, ox = p - oy * a.W;
    const bool second = n >= (size_t)a.N;
    const void* src = second ? a.b : a.a;
    const bool u8 = second ? a.u8b != 0 : a.u8a != 0;
    const size_t img = second ? n - (size_t)a.N : n;
    const LpConstF wc = (LpConstF)a.w;

    float v[VG_HEAD_K];   // the 27 samples first, so that their loads are in flight together
#pragma unroll
    for (int ci = 0; ci < 3; ++ci) {
        const float shift = wc[VG_HEAD_SS + ci], scale = wc[VG_HEAD_SS + 4 + ci];
#pragma unroll
        for (int kh = 0; kh < 3; ++kh) {
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                const int iy = oy - 1 + kh, ix = ox - 1 + kw;
                float s = 0.0f;   // the convolution's padding is zero AFTER the scaling layer
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    const size_t pix = (size_t)iy * a.W + ix;
                    if (u8) s = d_u8(static_cast<const unsigned char*>(src)[(img * HW + pix) * 3 + ci]);
                    else s = static_cast<const float*>(src)[(img * 3 + ci) * HW + pix];
                    if (a.unit) s = s * 0.5f + 0.5f;
                    if (a.scaled) s = (s - shift) / scale;
                }
                v[(ci * 3 + kh) * 3 + kw] = s;
            }
        }
    }
    float acc[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) acc[j] = 0.0f;
#pragma unroll
    for (int k = 0; k < VG_HEAD_K; ++k) {
        const LpConstF wk = wc + k * 64;
#pragma unroll
        for (int j = 0; j < 64; ++j) acc[j] = fmaf(wk[j], v[k], acc[j]);
    }
    if (valid) {
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
            float* dst = a.out + ((n * 8 + (size_t)cb) * HW + p) * 8;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                d_f32x4 y;
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = lp_relu(acc[cb * 8 + h * 4 + r] + wc[VG_HEAD_B + cb * 8 + h * 4 + r]);
                *reinterpret_cast<d_f32x4*>(dst + h * 4) = y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Content loss: out[n] = mean over the 256 * H3 * W3 values of (relu3_3(a_n) - relu3_3(b_n))^2.  Thread t sums elements 4 t ... 4 t + 3,
// then every 4 * D_THREADS-th group after them, in memory order of the C8 tensor; the 256 partial sums meet in a tree.
struct VgContentArgs {
    const float* tap;    // relu3_3: C8, 256 channels, 2 N images
    double* out;         // [N]
    long long count;     // 256 * H3 * W3
    int N;
};

__global__ void __launch_bounds__(D_THREADS) k_vgg_content(const VgContentArgs a) {
    __shared__ double red[D_THREADS];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x;
    const float* fa = a.tap + n * (size_t)a.count;
    const float* fb = a.tap + (n + (size_t)a.N) * (size_t)a.count;
    double part = 0.0;
    for (long long i = (long long)tid * 4; i < a.count; i += 4 * D_THREADS) {
        const d_f32x4 u = *reinterpret_cast<const d_f32x4*>(fa + i), v = *reinterpret_cast<const d_f32x4*>(fb + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double t = (double)u[e] - (double)v[e];
            part += t * t;
        }
    }
    red[tid] = part;
    __syncthreads();
    for (int s = D_THREADS / 2; s > 0; s >>= 1) {
        if (tid < s) red[tid] += red[tid + s];
        __syncthreads();
    }
    if (tid == 0) a.out[n] = red[0] / (double)a.count;
}

}  // namespace cid
