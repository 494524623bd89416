// srgan_disc_bwd_kernels.h — gfx950 device kernels of the SRGAN trainer's discriminator backward pass (cid_srd_backward,
// include/cid.h), reference backend/trainingcode/srgan_code/sr_ganTrainGNew.py:54-80.
//
// model.0 ... model.10 are the denoise discriminator's layers and their gradients run on the kernels of disc_bwd_kernels.h unchanged
// (BatchNorm 9 with a tensor upstream).  model.11 and BatchNorm 12 run on that file's k_disc_wgrad, k_disc_dgrad and
// k_disc_bn_bwd_part with POOL and the part arguments set.  What this file adds is the head, from what cid_srd_forward_saved kept
// per image in fp64: the 256 pooled means m of a12 and the 512 hidden pre-activations h = W15 m + b15.
//   * k_srd_head_bwd: one 512-thread workgroup per image.
//         a16 = lrelu(h)    p = sigmoid(b17 + sum_j w17[j] * a16[j])    dl = grad_prob * p * (1 - p)
//         dh[j] = dl * w17[j] * (h[j] > 0 ? 1 : 0.2)                    dm[c] = sum_j dh[j] * W15[j][c]
//     The slope decision is the forward's, on the same fp64 value.  It writes dl, dh (fp64) and up[n][c] = (float)(dm[c] / P): the
//     gradient of every pixel of a12's channel c of image n, which BatchNorm 12's consumers read as D_UP_POOL.
//   * k_srd_head_reduce: the sums over images, in image order, in fp64: dW15[j][c] = sum_n dh[n][j] * m[n][c] (a workgroup owns
//     eight j and all 256 c), and in one more workgroup db15[j] = sum_n dh[n][j], dw17[j] = sum_n dl[n] * a16[n][j], db17 = sum_n dl[n].
//   * k_srd_hidden_mask: testing aid, h > 0 as the kernels above decide it.
// The device pack of its fourteen parameter tensors is k_disc_pack (disc_bwd_kernels.h).
#pragma once
#include "disc_bwd_kernels.h"
#include "srgan_disc_kernels.h"

namespace cid {

constexpr int SRD_HB_THREADS = SRD_HEAD_HID;

struct SrdHeadBwdArgs {
    const double* hidden;    // [N][512]
    const float* w1;         // model.15: [512][256], then the biases
    const float* w2;         // model.17: [512], then the bias
    const float* grad_prob;  // [N]
    double* dl;              // out [N]
    double* dh;              // out [N][512]
    float* up;               // out [N][256]: dm / P
    double P;
    int n0;
};

__global__ void __launch_bounds__(SRD_HB_THREADS) k_srd_head_bwd(const SrdHeadBwdArgs a) {
    static_assert(SRD_HB_THREADS == 2 * SRD_HEAD_C, "two halves of the hidden units per channel");
    __shared__ double red[SRD_HEAD_HID];
    __shared__ double dhs[SRD_HEAD_HID];
    const int tid = threadIdx.x;
    const size_t n = (size_t)a.n0 + blockIdx.x;
    const double h = a.hidden[n * SRD_HEAD_HID + tid];
    const double w2 = (double)a.w2[tid];
    red[tid] = w2 * (h > 0.0 ? h : h * 0.2);
    __syncthreads();
    for (int off = SRD_HEAD_HID / 2; off > 0; off >>= 1) {   // the forward's tree
        if (tid < off) red[tid] += red[tid + off];
        __syncthreads();
    }
    const double logit = (double)a.w2[SRD_HEAD_HID] + red[0];
    const double p = 1.0 / (1.0 + exp(-logit));
    const double dl = (double)a.grad_prob[n] * p * (1.0 - p);
    const double dh = dl * w2 * (h > 0.0 ? 1.0 : 0.2);
    dhs[tid] = dh;
    a.dh[n * SRD_HEAD_HID + tid] = dh;
    if (tid == 0) a.dl[n] = dl;
    __syncthreads();
    // dm[c]: thread (half, c) adds its 256 hidden units in order, then the two halves meet
    const int c = tid & (SRD_HEAD_C - 1), half = tid / SRD_HEAD_C;
    const float* col = a.w1 + (size_t)half * (SRD_HEAD_HID / 2) * SRD_HEAD_C + c;
    double s = 0.0;
    for (int j = 0; j < SRD_HEAD_HID / 2; ++j) s += dhs[half * (SRD_HEAD_HID / 2) + j] * (double)col[(size_t)j * SRD_HEAD_C];
    red[tid] = s;   // red[0] was read by every thread before the barrier above
    __syncthreads();
    if (tid < SRD_HEAD_C) a.up[n * SRD_HEAD_C + tid] = (float)((red[tid] + red[tid + SRD_HEAD_C]) / a.P);
}

constexpr int SRD_HR_J = 8;                              // hidden units per workgroup of the dW15 sum
constexpr int SRD_HR_BLOCKS = SRD_HEAD_HID / SRD_HR_J;   // + 1 workgroup for the three vectors

struct SrdHeadReduceArgs {
    const double* pooled;   // [N][256]
    const double* hidden;   // [N][512]
    const double* dl;       // [N]
    const double* dh;       // [N][512]
    float* dw15;            // out [512][256], may be null
    float* db15;            // out [512], may be null
    float* dw17;            // out [512], may be null
    float* db17;            // out [1], may be null
    int N;
};

__global__ void __launch_bounds__(SRD_HEAD_C) k_srd_head_reduce(const SrdHeadReduceArgs a) {
    const int tid = threadIdx.x;
    if (blockIdx.x < SRD_HR_BLOCKS) {
        if (!a.dw15) return;
        const int j0 = blockIdx.x * SRD_HR_J;
        double acc[SRD_HR_J];
#pragma unroll
        for (int u = 0; u < SRD_HR_J; ++u) acc[u] = 0.0;
        for (int n = 0; n < a.N; ++n) {
            const double m = a.pooled[(size_t)n * SRD_HEAD_C + tid];
            const double* dh = a.dh + (size_t)n * SRD_HEAD_HID + j0;
#pragma unroll
            for (int u = 0; u < SRD_HR_J; ++u) acc[u] += dh[u] * m;
        }
#pragma unroll
        for (int u = 0; u < SRD_HR_J; ++u) a.dw15[(size_t)(j0 + u) * SRD_HEAD_C + tid] = (float)acc[u];
        return;
    }
    for (int j = tid; j < SRD_HEAD_HID; j += SRD_HEAD_C) {
        if (a.db15) {
            double s = 0.0;
            for (int n = 0; n < a.N; ++n) s += a.dh[(size_t)n * SRD_HEAD_HID + j];
            a.db15[j] = (float)s;
        }
        if (a.dw17) {
            double s = 0.0;
            for (int n = 0; n < a.N; ++n) {
                const double h = a.hidden[(size_t)n * SRD_HEAD_HID + j];
                s += a.dl[n] * (h > 0.0 ? h : h * 0.2);
            }
            a.dw17[j] = (float)s;
        }
    }
    if (a.db17 && tid == 0) {
        double s = 0.0;
        for (int n = 0; n < a.N; ++n) s += a.dl[n];
        a.db17[0] = (float)s;
    }
}

// Testing aid: LeakyReLU's mask of the hidden layer, uint8 [N][512] (1 where the slope is 1).
__global__ void __launch_bounds__(D_THREADS) k_srd_hidden_mask(const double* hidden, unsigned char* out, long long total) {
    const long long o = (long long)blockIdx.x * D_THREADS + threadIdx.x;
    if (o < total) out[o] = hidden[o] > 0.0 ? 1 : 0;
}

}  // namespace cid
