// srgan_disc_kernels.h — gfx950 device kernels of the SRGAN trainer's discriminator forward (cid_srd_forward, include/cid.h),
// reference backend/trainingcode/srgan_code/sr_ganTrainGNew.py:54-80.
//
// model.0 ... model.10 are the denoise trainer's discriminator: the layer-0 kernel, the MFMA convolution k_disc_conv, the train-mode
// statistics kernel and the C8 layout of disc_kernels.h serve them unchanged.  What this file adds:
//   * model.11, Conv2d(128, 256, 3, p=1), is k_disc_conv<128, 128, 1, true, STATS, 256>: the kernel keeps its 128-channel workgroup
//     and the layer runs as two channel halves, grid z = half (disc_kernels.h).  No kernel text here.
//   * The eval-mode (scale, shift) of its four BatchNorms and their counters' increment are k_disc_bn_eval and k_disc_bn_count, which
//     take up to four BatchNorms of up to 256 channels.  No kernel text here either.
//   * k_srd_head: one 1024-thread workgroup per image: BN12 + LeakyReLU of z11, the global average, Conv2d(256, 512, 1) + LeakyReLU,
//     Conv2d(512, 1, 1) and the sigmoid, every sum in fp64 in a fixed order.
//   * k_srd_losses: the SRGAN trainer's two BCE reductions over one batch (fp64, fixed order).
//   * k_srd_head_saved: what cid_srd_forward_saved runs in k_srd_head's place.  It also keeps the 256 pooled means and the 512 hidden
//     pre-activations of each image, in fp64, for the backward's head (srgan_disc_bwd_kernels.h), and shares the plain kernel's
//     arithmetic statement for statement.
#pragma once
#include "disc_kernels.h"

namespace cid {

// ---------------------------------------------------------------------------------------------------------------------------
// Head: BatchNorm12 + LeakyReLU of z11, AdaptiveAvgPool2d(1), Conv2d(256, 512, 1) + LeakyReLU, Conv2d(512, 1, 1), Sigmoid.
// One 1024-thread workgroup per image, three phases:
//   pool     wave w takes the channel blocks 2w and 2w + 1 of the C8 tensor, one after the other.  Lane l reads the four channels of half
//            l % 2 of pixels l / 2, l / 2 + 32, ... (one 16-byte load each, a wave's 64 loads are 1 KiB of consecutive memory, four
//            of them in flight), adds them in that order and the 32 pixel lanes meet in a butterfly.
//   hidden   wave w computes the 32 hidden units 32*w ... 32*w + 31, one after the other: lane l multiplies channels l, l + 64, l + 128,
//            l + 192 of the unit's weight row (a coalesced 1 KiB read) with the pooled means and the 64 lane sums meet in a butterfly.
//   logit    512 products reduced by a tree.
// Every sum is fp64 in an order that depends on P alone, never on N or on the image's position in the batch.
constexpr int SRD_HEAD_THREADS = 1024;
constexpr int SRD_HEAD_C = 256;
constexpr int SRD_HEAD_HID = 512;
constexpr int SRD_HEAD_PL = 32;   // pixel lanes of the pool
struct SrdHeadArgs {
    const float* z;     // z11, C8, 256 channels, P = H4 * W4 pixels per image
    const float* st;    // BN12 (scale, shift) pairs [256]
    const float* w1;    // model.15: [512][256] reference order, then the 512 biases
    const float* w2;    // model.17: [512], then the bias
    float* out;         // [N]
    long long P;
    int n0;
};

// Adds the four activated channels of one staged quad to their sums.
__device__ __forceinline__ void d_srd_pool_add(double (&acc)[4], const d_f32x4 v, const float (&s)[4], const float (&t)[4]) {
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[j] += (double)d_lrelu(d_bn(s[j], v[j], t[j]));
}

// SAVE: the pooled means go to pooled_out[n][256] and the hidden pre-activations to hidden_out[n][512] as well.
template <bool SAVE>
__device__ __forceinline__ void d_srd_head(const SrdHeadArgs& a, double* pooled_out, double* hidden_out) {
    static_assert(SRD_HEAD_C / 8 == 2 * (SRD_HEAD_THREADS / 64), "two channel blocks per wave");
    __shared__ double red[SRD_HEAD_HID];
    __shared__ double pooled[SRD_HEAD_C];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t n = (size_t)a.n0 + blockIdx.x;
    {
        const int half = lane & 1, pl = lane >> 1;
        for (int bi = 0; bi < 2; ++bi) {
            const int blk = wave * 2 + bi, c0 = blk * 8 + half * 4;
            float s[4], t[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                s[j] = a.st[2 * (c0 + j)];
                t[j] = a.st[2 * (c0 + j) + 1];
            }
            const float* zb = a.z + ((n * (SRD_HEAD_C / 8) + blk) * (size_t)a.P) * 8 + half * 4;
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            long long p = pl;
            for (; p + 3 * SRD_HEAD_PL < a.P; p += 4 * SRD_HEAD_PL) {
                d_f32x4 v[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const d_f32x4*>(zb + (p + u * SRD_HEAD_PL) * 8);
#pragma unroll
                for (int u = 0; u < 4; ++u) d_srd_pool_add(acc, v[u], s, t);
            }
            for (; p < a.P; p += SRD_HEAD_PL) d_srd_pool_add(acc, *reinterpret_cast<const d_f32x4*>(zb + p * 8), s, t);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int off = 2; off < 64; off <<= 1) acc[j] += __shfl_xor(acc[j], off, 64);
                if (pl == 0) {
                    pooled[c0 + j] = acc[j] / (double)a.P;
                    if (SAVE) pooled_out[n * SRD_HEAD_C + c0 + j] = pooled[c0 + j];
                }
            }
        }
    }
    __syncthreads();
    double mine[SRD_HEAD_C / 64];
#pragma unroll
    for (int k = 0; k < SRD_HEAD_C / 64; ++k) mine[k] = pooled[lane + 64 * k];
    constexpr int PER_WAVE = SRD_HEAD_HID / (SRD_HEAD_THREADS / 64);
#pragma unroll 4
    for (int u = 0; u < PER_WAVE; ++u) {
        const int j = wave * PER_WAVE + u;
        const float* row = a.w1 + (size_t)j * SRD_HEAD_C;
        double acc = 0.0;
#pragma unroll
        for (int k = 0; k < SRD_HEAD_C / 64; ++k) acc += (double)row[lane + 64 * k] * mine[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) {
            const double h = acc + (double)a.w1[SRD_HEAD_HID * SRD_HEAD_C + j];
            red[j] = (double)a.w2[j] * (h > 0.0 ? h : h * 0.2);
            if (SAVE) hidden_out[n * SRD_HEAD_HID + j] = h;
        }
    }
    __syncthreads();
    for (int off = SRD_HEAD_HID / 2; off > 0; off >>= 1) {
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    if (tid == 0) {
        const double logit = (double)a.w2[SRD_HEAD_HID] + red[0];
        a.out[n] = (float)(1.0 / (1.0 + exp(-logit)));
    }
}

__global__ void __launch_bounds__(SRD_HEAD_THREADS) k_srd_head(const SrdHeadArgs a) { d_srd_head<false>(a, nullptr, nullptr); }

struct SrdHeadSavedArgs {
    SrdHeadArgs head;
    double* pooled;   // out [N][256]
    double* hidden;   // out [N][512]
};

__global__ void __launch_bounds__(SRD_HEAD_THREADS) k_srd_head_saved(const SrdHeadSavedArgs a) {
    d_srd_head<true>(a.head, a.pooled, a.hidden);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The SRGAN trainer's adversarial losses of one batch (sr_ganTrainGNew.py:395-407): one workgroup, fp64, fixed order.
//   out[0] d_loss = BCE(p_real, 1) + BCE(p_fake, 0)    out[1] adv_loss = BCE(p_fake, 1)
struct SrdLossArgs {
    const float* p_real;
    const float* p_fake;
    int N;
    double* out;
};

__global__ void __launch_bounds__(D_LOSS_THREADS) k_srd_losses(const SrdLossArgs a) {
    __shared__ double red[D_LOSS_THREADS];
    const int tid = threadIdx.x;
    double real1 = 0.0, fake0 = 0.0, fake1 = 0.0;
    for (int i = tid; i < a.N; i += D_LOSS_THREADS) d_bce_terms(a.p_real[i], a.p_fake[i], real1, fake0, fake1);
    real1 = d_block_sum(real1, red);
    fake0 = d_block_sum(fake0, red);
    fake1 = d_block_sum(fake1, red);
    if (tid == 0) {
        a.out[0] = real1 / a.N + fake0 / a.N;
        a.out[1] = fake1 / a.N;
    }
}

}  // namespace cid
