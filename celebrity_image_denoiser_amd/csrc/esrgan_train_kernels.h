// esrgan_train_kernels.h — gfx950 device kernels of the ESRGAN generator's forward in TRAIN mode (cid_esr_forward_train, include/cid.h):
// the first line of the ESRGAN trainer's step, denoised = G(noisy) after G.train() (backend/trainingcode/esrgan_code/esrgan_train.py:89-121),
// with BatchNorm on batch statistics, fp32.  With R residual blocks, r_{-1} = x1:
//
//     x1       = PReLU(Conv2d(3, 64, 9, pad 4)(x))                              k_esr_head (esrgan_kernels.h)
//     z_0      = Conv3x3(x1) + bias                                             k_sr_train_conv<ST_IN_RAW, ST_EPI_STATS>
//     z_{2i+1} = Conv3x3(PReLU(BN_{2i}(z_{2i}))) + bias                         k_sr_train_conv<ST_IN_BN_PRELU, ST_EPI_STATS>
//     r_i      = r_{i-1} + BN_{2i+1}(z_{2i+1})                                  formed and stored by the launch below
//     z_{2i+2} = Conv3x3(r_i) + bias                                            k_esr_train_conv (ST_IN_RES_BN, ST_EPI_STATS)
//     tail_in  = x1 + (r_{R-2} + BN_{2R-1}(z_{2R-1}))                           k_esr_train_sum
//     out      = Conv2d(64, 3, 9, pad 4)(tail_in)                               k_esr_tail (esrgan_kernels.h)
//
// The block's skip needs BN_{2i+1}'s statistics, which exist only once the convolution that makes z_{2i+1} has finished over the whole
// batch: the sum cannot be that convolution's epilogue, as it is in eval mode (k_esr_conv<EPI_RES>).  The NEXT convolution forms
// r_i = res + fmaf(scale, z, shift) (eval's expression and association) while it stages its halo, and the workgroup that owns a pixel
// (its tile's 16 x 16 interior, not the halo ring) also stores it: every element of r_i is written exactly once, and the values the
// neighbouring tiles recompute for their halos have the same bits.  A launch never stores to the tensor it reads `res` from, because
// neighbours read that tensor's halo: the host alternates the r_i between two tensors and keeps x1 apart.
//
// The tile is sr_train_conv_tile (srgan_train_kernels.h): LDS layout, chunk loop, exact-fp32 MFMA, chunk-wise partial sums and the
// STATS epilogue are those of the SRGAN generator's train-mode forward.  No atomics, every sum in a fixed order, 64-bit offsets.
#pragma once
#include <hip/hip_runtime.h>

#include "srgan_train_kernels.h"

namespace cid {

constexpr int E_TRAIN_MAX_BNS = 32;   // residuals.i.block.1, residuals.i.block.4, i = 0 .. 15

// Its own struct and kernel: the four instantiations of k_sr_train_conv keep their arguments and their registers.
struct EsrTrainConvArgs {
    SrTrainConvArgs c;    // in = the previous convolution's raw z; st_in = its BatchNorm's (scale, shift); res and slope are not read
    const float* res_in;  // C8: the previous block's output (x1 for the first block)
    float* r_out;         // C8: res_in + BN(z), never the tensor behind res_in
};

__global__ void __launch_bounds__(D_THREADS, 2) k_esr_train_conv(const EsrTrainConvArgs a) {
    sr_train_conv_tile<ST_IN_RES_BN, ST_EPI_STATS>(a.c, a.res_in, a.r_out);
}

// The tail's input from the last block: out = x1 + (res + fmaf(scale, z, shift)), the association of k_esr_conv<EPI_SUM>.  One thread
// per C8 quad (four consecutive channels of one pixel); grid = (quads of one image / D_THREADS, images).
struct EsrTrainSumArgs {
    const float* z;       // C8: the last convolution's raw result
    const float* res;     // C8: the last block's input (x1 where there is one block)
    const float* x1;      // C8
    float* out;           // C8
    const float* st;      // (scale, shift) pairs [64] of the last BatchNorm
    long long plane;      // H * W
    int n0;
};

__global__ void __launch_bounds__(D_THREADS) k_esr_train_sum(const EsrTrainSumArgs a) {
    const size_t q = (size_t)blockIdx.x * D_THREADS + threadIdx.x;   // quad inside the image: (channel block * plane + pixel) * 2 + half
    const size_t quads = (size_t)a.plane * 16;
    if (q >= quads) return;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int c = (int)(q / ((size_t)a.plane * 2)) * 8 + (int)(q & 1) * 4;   // first of the quad's four channels
    const size_t at = (n * quads + q) * 4;
    const d_f32x4 z = *reinterpret_cast<const d_f32x4*>(a.z + at);
    const d_f32x4 r = *reinterpret_cast<const d_f32x4*>(a.res + at);
    const d_f32x4 x = *reinterpret_cast<const d_f32x4*>(a.x1 + at);
    const d_f32x4 s0 = *reinterpret_cast<const d_f32x4*>(a.st + 2 * c);       // scale, shift of channels c, c + 1
    const d_f32x4 s1 = *reinterpret_cast<const d_f32x4*>(a.st + 2 * c + 4);   // and of c + 2, c + 3
    d_f32x4 y;
    y[0] = d_bn(s0[0], z[0], s0[1]);
    y[1] = d_bn(s0[2], z[1], s0[3]);
    y[2] = d_bn(s1[0], z[2], s1[1]);
    y[3] = d_bn(s1[2], z[3], s1[3]);
    y = r + y;
    *reinterpret_cast<d_f32x4*>(a.out + at) = x + y;
}

// num_batches_tracked += 1 of the 2 R BatchNorms, after every statistics launch has read them.
struct EsrBnCountArgs {
    long long* count[E_TRAIN_MAX_BNS];
    int n;
};

__global__ void __launch_bounds__(64) k_esr_bn_count(const EsrBnCountArgs a) {
#pragma unroll
    for (int i = 0; i < E_TRAIN_MAX_BNS; ++i)   // unrolled: the pointers stay in scalar registers
        if ((int)threadIdx.x == i && i < a.n) a.count[i][0] += 1;
}

}  // namespace cid
