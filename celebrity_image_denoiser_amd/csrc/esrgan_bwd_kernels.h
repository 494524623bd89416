// esrgan_bwd_kernels.h — gfx950 device kernels of the ESRGAN generator's backward pass in train mode (cid_esr_backward, include/cid.h):
// the gradients of every parameter of esrgan_train_kernels.h's network from grad_out [N,3,H,W] and what cid_esr_forward_saved kept: the
// head's pre-activation v0 (k_esr_head<U8, true>, esrgan_kernels.h), the 2 R raw z_l, the block outputs r_0 .. r_{R-2}, tail_in and each
// BatchNorm's (scale, shift) and (mean, invstd).
//
// The GEMM-shaped and the reducing kernels are srgan_bwd_kernels.h's templates, fp32 in the C8 layout, every reduction in fp64 in a
// fixed order through a slab and a reduce launch, no atomics, 64-bit offsets.  The instantiations this graph adds to the SRGAN
// generator's are k_srg_wgrad<SG_DZ_BN, SG_IN_RAW> (a block's first convolution reads the previous block's stored output) and
// k_srg_tail_wgrad<false> on tail_in with raw = 1, and k_srg_wgrad243<true>, which reads a uint8 input as this head does (u / 255);
// what is new here is
//   * k_esrg_join: the gradient of x1 from its consumers.  x1 feeds block 0 (convolution 0 and the block's skip, whose sum
//     G_{-1} = G_0 + dgrad_0 leaves k_srg_dgrad with add = G_0, in that order) and the outer skip into tail_in (dT):
//     d x1 = G_{-1} + dT, in that order; with R = 0, tail_in = x1 + x1 and d x1 = dT + dT.
//   * k_esrg_pack: the forward's packed blob for R blocks from the parameter tensors and the running statistics on the device.
#pragma once
#include <hip/hip_runtime.h>

#include "esrgan_train_kernels.h"
#include "srgan_bwd_kernels.h"

namespace cid {

// out = g + dT (g null: dT + dT).  One thread per C8 quad; grid = (quads of one image / D_THREADS, images).
struct EsrgJoinArgs {
    const float* g;       // C8: G_{-1}, the gradient that reaches x1 through block 0; null with R = 0
    const float* dT;      // C8: the gradient of tail_in
    float* out;           // C8: the gradient of x1
    long long quads;      // 16 * H * W
    int n0;
};

__global__ void __launch_bounds__(D_THREADS) k_esrg_join(const EsrgJoinArgs a) {
    const size_t q = (size_t)blockIdx.x * D_THREADS + threadIdx.x;
    if (q >= (size_t)a.quads) return;
    const size_t at = (((size_t)a.n0 + blockIdx.y) * (size_t)a.quads + q) * 4;
    const d_f32x4 t = *reinterpret_cast<const d_f32x4*>(a.dT + at);
    *reinterpret_cast<d_f32x4*>(a.out + at) = (a.g ? *reinterpret_cast<const d_f32x4*>(a.g + at) : t) + t;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The forward's packed blob from the parameter tensors (reference layouts, device memory) and the BatchNorm running buffers: what
// cid_esr_set_weight + cid_esr_upload_weights build on the host (esr_pack, api/esrgan.h), byte for byte, gaps (0) included.  Grid y is
// the segment: 0 head, 1 .. 2R the trunk convolutions, 2R + 1 the tail.  The eval-mode fold of BatchNorm l is pack_bn_fold's fp64
// arithmetic with its roundings spelt out (the host rounds mean * s before it subtracts), as in k_srg_pack.
struct EsrgPackArgs {
    const float* head_w;
    const float* head_b;
    const float* head_slope;
    const float* conv_w[E_TRAIN_MAX_BNS];   // residuals.i.block.{0,3}.weight at 2i, 2i+1
    const float* conv_b[E_TRAIN_MAX_BNS];
    const float* slope[E_TRAIN_MAX_BNS / 2];
    const float* gamma[E_TRAIN_MAX_BNS];
    const float* beta[E_TRAIN_MAX_BNS];
    const float* mean[E_TRAIN_MAX_BNS];
    const float* var[E_TRAIN_MAX_BNS];
    double eps[E_TRAIN_MAX_BNS];
    const float* tail_w;
    const float* tail_b;
    float* blob;
    int R;
};
static_assert(sizeof(EsrgPackArgs) <= 4096, "kernel arguments");

__global__ void __launch_bounds__(D_THREADS) k_esrg_pack(const EsrgPackArgs a) {
    const int seg = blockIdx.y, r = blockIdx.x * D_THREADS + threadIdx.x;
    float v = 0.0f;
    if (seg == 0) {
        if (r >= SG_PACK_HEAD) return;
        if (r < E_HEAD_K * 64) v = a.head_w[(r % 64) * E_HEAD_K + r / 64];
        else if (r < E_HEAD_K * 64 + 64) v = a.head_b[r - E_HEAD_K * 64];
        else if (r == E_HEAD_K * 64 + 64) v = a.head_slope[0];
        a.blob[r] = v;
    } else if (seg <= 2 * a.R) {
        if (r >= SG_PACK_CONV) return;
        const int l = seg - 1;
        if (r < E_CONV_W) {
            const int co = r % 64, q = r / 64, ci8 = q & 7, tap = (q >> 3) % 9, chunk = (q >> 3) / 9;
            v = a.conv_w[l][((size_t)co * 64 + chunk * 8 + ci8) * 9 + tap];
        } else if (r < E_CONV_S) {
            v = a.conv_b[l][r - E_CONV_BIAS];
        } else if (r < E_CONV_SLOPE) {
            const bool is_t = r >= E_CONV_T;
            const int ch = r - (is_t ? E_CONV_T : E_CONV_S);
            const double s = (double)a.gamma[l][ch] / sqrt((double)a.var[l][ch] + a.eps[l]);
            v = is_t ? (float)__dsub_rn((double)a.beta[l][ch], __dmul_rn((double)a.mean[l][ch], s)) : (float)s;
        } else if (r == E_CONV_SLOPE && l % 2 == 0) {
            v = a.slope[l / 2][0];
        }
        a.blob[SG_PACK_HEAD + (size_t)l * SG_PACK_CONV + r] = v;
    } else {
        if (r >= SG_PACK_TAIL) return;
        if (r < E_TAIL_W) {
            const int col = r % E_TAIL_WROW, q = r / E_TAIL_WROW, kh = q % 9, ci = q / 9;
            if (col < 27) v = a.tail_w[(((size_t)(col / 9) * 64 + ci) * 9 + kh) * 9 + col % 9];
        } else if (r < E_TAIL_W + 3) {
            v = a.tail_b[r - E_TAIL_W];
        }
        a.blob[SG_PACK_HEAD + (size_t)2 * a.R * SG_PACK_CONV + r] = v;
    }
}

}  // namespace cid
