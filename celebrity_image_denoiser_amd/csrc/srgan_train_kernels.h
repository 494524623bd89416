// srgan_train_kernels.h — gfx950 device kernels of the SRGAN generator's forward in TRAIN mode (cid_sr_forward_train, include/cid.h):
// the trunk of backend/trainingcode/srgan_code/sr_ganTrainGNew.py:19-51 with BatchNorm on batch statistics, fp32.
//
//     x0  = PReLU(Conv2d(3, 64, 9, pad 4)(x))                                   k_sr_head (srgan_kernels.h)
//     z_0 = Conv3x3(x0) + bias                                                  k_sr_train_conv<ST_IN_RAW, ST_EPI_STATS>
//     z_l = Conv3x3(PReLU(BN_{l-1}(z_{l-1}))) + bias      l = 1, 3, 5, 7, 9     k_sr_train_conv<ST_IN_BN_PRELU, ST_EPI_STATS>
//     z_l = Conv3x3(BN_{l-1}(z_{l-1})) + bias             l = 2, 4, 6, 8        k_sr_train_conv<ST_IN_BN, ST_EPI_STATS>
//     t   = x0 + Conv3x3(BN_9(z_9)) + bias                mid                   k_sr_train_conv<ST_IN_BN, ST_EPI_RES>
//     upscale stages and tail                                                   k_sr_up, k_sr_tail (srgan_kernels.h)
//
// BN_l is the l-th BatchNorm (res_blocks.(l/2).(1 or 4)) on the statistics of THIS batch.  A convolution stores its raw result z_l and
// its per-tile, per-channel sums of z and z^2 in fp64 to its own row of a slab; k_disc_bn_stats (disc_kernels.h) reduces the slab in a
// fixed order to the layer's (scale, shift) and updates the running buffers; the NEXT convolution applies y = fmaf(scale, z, shift)
// (d_bn) and, where the block has one there, PReLU (e_prelu) once per element while it stages its halo.  Halo positions outside the
// image are the zero padding of the ACTIVATED tensor: 0, not BN(0).
//
// k_sr_train_conv is the 16 x 16-pixel, 64-channel tile of k_esr_conv / k_disc_conv<64, 64, 1>: the same LDS layout (DiscGeom), chunk
// loop and exact-fp32 MFMA (v_mfma_f32_16x16x4_f32), the STATS epilogue of k_disc_conv; unlike them it sums each 8-channel chunk on
// its own (below).  No atomics, every sum in a fixed order, 64-bit offsets (a pixel index inside one image is an int), an image's
// tiles depend only on (H, W).
#pragma once
#include <hip/hip_runtime.h>

#include "esrgan_kernels.h"

namespace cid {

// what the staging applies to the input; ST_IN_RES_BN is the ESRGAN generator's (esrgan_train_kernels.h): res + BN(z), stored as well
enum { ST_IN_RAW = 0, ST_IN_BN = 1, ST_IN_BN_PRELU = 2, ST_IN_RES_BN = 3 };
enum { ST_EPI_STATS = 0, ST_EPI_RES = 1 };                  // z + slab row, or res + z

constexpr int S_TRAIN_BNS = 10;   // res_blocks.i.1, res_blocks.i.4, i = 0 .. 4

struct SrTrainConvArgs {
    const float* in;      // C8, 64 channels: x0 (ST_IN_RAW) or the previous convolution's raw z
    float* out;           // C8, 64 channels: z = conv + bias (ST_EPI_STATS) or res + conv + bias (ST_EPI_RES)
    const float* res;     // ST_EPI_RES: x0
    const float* w;       // the convolution's blob segment (EsrConvArgs::w): packed weights, then the 64 biases; the folded
                          // (s, t) behind them belong to eval mode and are not read
    const float* st_in;   // ST_IN_BN, ST_IN_BN_PRELU: (scale, shift) pairs [64] of the previous BatchNorm
    const float* slope;   // ST_IN_BN_PRELU: the block's PReLU slope (one float of the blob)
    double* slab;         // ST_EPI_STATS: slab[(co*2 + k)*rows + row], k = 0: sum z, 1: sum z^2; row = image * tiles + tile
    long long rows;
    int H, W;
    int tiles_x, tiles;   // tiles per tile row / per image
    int n0;
};

// The tile itself, shared with k_esr_train_conv (esrgan_train_kernels.h).  ST_IN_RES_BN only: `res_in` is the tensor the staged
// BatchNorm is added to and `r_out` the tensor that sum is stored to, both C8 like `a.in`; the other modes pass null and read neither.
// `a` comes by value, as a kernel's own argument does: by reference the STATS instantiations take one more SGPR.
template <int IN, int EPI>
__device__ __forceinline__ void sr_train_conv_tile(const SrTrainConvArgs a, const float* res_in, float* r_out) {
    using G = DiscGeom<64, 64, 1>;
    constexpr int WM = G::WM, TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    constexpr bool STATS = EPI == ST_EPI_STATS;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];
    __shared__ float lds_st[IN != ST_IN_RAW ? 2 * 64 : 1];
    __shared__ double lds_red[STATS ? WM * 64 * 2 : 1];

    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int iy0 = ty * TH - 1, ix0 = tx * D_TW - 1;
    const size_t plane = (size_t)a.H * a.W;

    if (IN != ST_IN_RAW)
        for (int i = tid; i < 2 * 64; i += D_THREADS) lds_st[i] = a.st_in[i];
    const float slope = IN == ST_IN_BN_PRELU ? a.slope[0] : 0.0f;

    // A chunk's 72 terms are summed on their own and then added to the total, as k_esr_tail does: a shorter rounding chain than 576 in
    // a row.  Train mode divides by the batch's own deviation ten times in a row, so a convolution's rounding error is carried, at
    // full scale, into every later layer.
    d_f32x4 acc[4][4], part[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * 4) * HWD + l16;   // this lane's B operand base (plane kq, its pixel column)
    const int wb = kq * WSTR + l16;                    // this lane's A operand base (row kq, its channel)

    for (int chunk = 0; chunk < 8; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk (and lds_st is visible before the first one)
        // ---- halo of this chunk: global -> VGPR -> (the previous BatchNorm, PReLU) -> LDS planes
        const float* src = a.in + ((n * 8 + chunk) * plane) * 8;
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int iy = iy0 + hy, ix = ix0 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};   // outside the image: the zero padding of the activated tensor
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                    v = *reinterpret_cast<const d_f32x4*>(src + ((size_t)iy * a.W + ix) * 8 + h * 4);
                    if (IN != ST_IN_RAW) {
                        const int c = chunk * 8 + h * 4;
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            v[j] = d_bn(lds_st[2 * (c + j)], v[j], lds_st[2 * (c + j) + 1]);
                            if (IN == ST_IN_BN_PRELU) v[j] = e_prelu(v[j], slope);
                        }
                    }
                    if (IN == ST_IN_RES_BN) {
                        // the block's output res + BN(z), eval's association; the tile that owns the pixel (its interior, not the
                        // halo ring) stores it, and every neighbour that stages the pixel computes the same bits
                        const size_t at = ((n * 8 + chunk) * plane + (size_t)iy * a.W + ix) * 8 + h * 4;
                        v = *reinterpret_cast<const d_f32x4*>(res_in + at) + v;
                        if (hy >= 1 && hy <= TH && hx >= 1 && hx <= D_TW) *reinterpret_cast<d_f32x4*>(r_out + at) = v;
                    }
                }
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
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int pt = 0; pt < 4; ++pt) part[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
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
                    for (int pt = 0; pt < 4; ++pt) part[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], part[ct][pt], 0, 0, 0);
            }
        }
#pragma unroll
        for (int ct = 0; ct < 4; ++ct)
#pragma unroll
            for (int pt = 0; pt < 4; ++pt) acc[ct][pt] += part[ct][pt];
    }

    // ---- epilogue: + bias; z and its per-channel partial sums, or the residual sum; four consecutive channels of one pixel per lane
    const int ox = tx * D_TW + l16;
    bool ok[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) ok[pt] = (ty * TH + wm * 4 + pt) < a.H && ox < a.W;
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int co = ct * 16 + kq * 4;   // first of this lane's four channels
        const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(a.w + E_CONV_BIAS + co);
        double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            d_f32x4 z = acc[ct][pt] + b4;
            if (ok[pt]) {
                const int oy = ty * TH + wm * 4 + pt;
                const size_t at = (((n * 8 + co / 8) * a.H + oy) * (size_t)a.W + ox) * 8 + (co & 7);
                if (!STATS) z = *reinterpret_cast<const d_f32x4*>(a.res + at) + z;
                *reinterpret_cast<d_f32x4*>(a.out + at) = z;
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
                    lds_red[(wm * 64 + co + r) * 2] = s1[r];
                    lds_red[(wm * 64 + co + r) * 2 + 1] = s2[r];
                }
            }
        }
    }
    if (STATS) {
        __syncthreads();
        if (tid < 64) {
            double t1 = 0.0, t2 = 0.0;
#pragma unroll
            for (int m = 0; m < WM; ++m) {
                t1 += lds_red[(m * 64 + tid) * 2];
                t2 += lds_red[(m * 64 + tid) * 2 + 1];
            }
            const long long row = (long long)n * a.tiles + t;
            a.slab[(size_t)(tid * 2) * a.rows + row] = t1;
            a.slab[(size_t)(tid * 2 + 1) * a.rows + row] = t2;
        }
    }
}

template <int IN, int EPI>
__global__ void __launch_bounds__(D_THREADS, 2) k_sr_train_conv(const SrTrainConvArgs a) {
    sr_train_conv_tile<IN, EPI>(a, nullptr, nullptr);
}

// num_batches_tracked += 1 of the ten BatchNorms, after every statistics launch has read them.
struct SrBnCountArgs {
    long long* count[S_TRAIN_BNS];
};

__global__ void __launch_bounds__(64) k_sr_bn_count(const SrBnCountArgs a) {
    if (threadIdx.x < S_TRAIN_BNS) a.count[threadIdx.x][0] += 1;
}

}  // namespace cid
