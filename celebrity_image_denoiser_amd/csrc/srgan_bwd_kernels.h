// srgan_bwd_kernels.h — gfx950 device kernels of the SRGAN generator's backward pass in train mode (cid_sr_backward, include/cid.h):
// the gradients of every parameter of srgan_train_kernels.h's network from grad_out [N,3,sH,sW] and what cid_sr_forward_saved kept:
// the head's pre-activation v0, the ten raw z_l, each BatchNorm's (scale, shift) and (mean, invstd), t, every upscale stage's
// pre-activation v_k (after the shuffle) and out.
//
// Tensors are fp32 in the forward's C8 layout.  Every reduction accumulates in fp64 in a fixed order through a slab and a reduce
// launch, no atomics; the GEMMs run on v_mfma_f32_16x16x4_f32 (exact fp32).  An image's tiling depends only on (H, W); offsets are
// 64-bit, a pixel index inside one image is an int.  The kernels follow disc_bwd_kernels.h (k_disc_dgrad, k_disc_wgrad,
// k_disc_bn_bwd_part / _reduce, k_disc_wgrad0) and share its geometry; what differs is the rule that forms dz, which is never stored
// but evaluated while an operand is staged:
//     SG_DZ_BN       y = d_bn(s, z, t); g = up * (y > 0 ? 1 : a); dz = k * (g - m1 - xh * m2)     a: coef slot 7 (1 where BN_l has no PReLU)
//     SG_DZ_PLAIN    dz = up                                                                     mid, whose result meets no BatchNorm
//     SG_DZ_PRELU    dz = up * (v > 0 ? 1 : a)                                                   the head
//     SG_DZ_SHUFFLE  dz[J] = up[co, 2y+i, 2x+j] * (v[co, 2y+i, 2x+j] > 0 ? 1 : a)                an upscale stage: packed column J of
//                    k_sr_up's GEMM is output channel co = 4 (J / 16) + J % 4, sub-pixel 2i + j = (J % 16) / 4; the 256-channel
//                    gradient exists only in LDS
// Every PReLU mask is decided on the saved PRE-activation, as e_prelu decides it (v > 0), so it is the forward's for any slope.
//   * k_srg_bn_part<DZ> + k_srg_bn_reduce + k_srg_sum: per-strip fp64 sums of g, g * xh and the slope's up * y over y <= 0; one
//     workgroup per channel reduces them to dgamma, dbeta, the coef table and the channel's share of the slope gradient, which
//     k_srg_sum adds up over the 64 channels.
//   * k_srg_dgrad<CD, DZ>: data gradient of a 3x3 convolution with 64 input channels (k_disc_dgrad, stride 1); CD = 256 reads k_sr_up's
//     packed columns.  `add` is a second gradient of the same tensor (x0's skip into t).
//   * k_srg_wgrad<DZ, IN, CD_TOTAL> + k_srg_wgrad_reduce: weight and bias gradient (k_disc_wgrad, stride 1); the staged input is a
//     tensor as it is, PReLU(v), BN(z) or PReLU(BN(z)); CD_TOTAL = 256 runs the stage's four 64-column parts in grid z and the
//     reduce maps packed columns back to convolution channels.
//   * k_srg_tail_dgrad: final's 3 -> 64 data gradient, K = (3, 9, 12): kw padded to three MFMA k-steps with zero weights.
//   * k_srg_wgrad243 + k_srg_wgrad243_reduce: the head's weight and bias gradient on the VALU in fp64, thread = (one of 64 channels,
//     a quarter of K = 244): dz x input patches (fp32 or uint8), K's last slot is the bias.  <true> reads uint8 as u / 255 (ESRGAN).
//   * k_srg_tail_wgrad<PRELU_IN>: final's weight gradient on the MFMA, 64 input channels x (co, kh) x kw per 4 x 16 pixel item; the
//     same reduce.
//   * k_srg_tail_bias_part: final's bias gradient.
//   * k_srg_pack: the forward's packed blob from the parameter tensors and the running statistics on the device.
#pragma once
#include <hip/hip_runtime.h>

#include "disc_bwd_kernels.h"
#include "srgan_train_kernels.h"

namespace cid {

enum { SG_DZ_BN = 0, SG_DZ_PLAIN = 1, SG_DZ_PRELU = 2, SG_DZ_SHUFFLE = 3 };
enum { SG_IN_RAW = 0, SG_IN_PRELU = 1, SG_IN_BN = 2, SG_IN_BN_PRELU = 3 };

struct SrgDz {
    const float* z;      // BN: the convolution's raw z; PRELU, SHUFFLE: the saved pre-activation; PLAIN: unused
    const float* up;     // gradient of the activated tensor, same shape as z
    const float* coef;   // BN: [64][D_COEF]; PRELU, SHUFFLE: the slope (one float)
};

// d(pre) of the tail from grad_out and out: tanh's derivative, or 1 with CID_SR_RAW.
__device__ __forceinline__ float sg_dpre(float g, float o, int raw) { return raw ? g : g * fmaf(-o, o, 1.0f); }

// Four consecutive channels (first channel c of the table in lds_cf) of dz at element offset `off`.
template <int DZ>
__device__ __forceinline__ d_f32x4 sg_dz4(const SrgDz& s, const float* lds_cf, size_t off, int c) {
    d_f32x4 u = *reinterpret_cast<const d_f32x4*>(s.up + off);
    if (DZ == SG_DZ_PLAIN) return u;
    const d_f32x4 z = *reinterpret_cast<const d_f32x4*>(s.z + off);
    d_f32x4 r;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (DZ == SG_DZ_BN) {
            const float* cf = lds_cf + (c + j) * D_COEF;
            const float g = u[j] * (d_bn(cf[0], z[j], cf[1]) > 0.0f ? 1.0f : cf[7]);
            r[j] = cf[2] * (g - cf[5] - (z[j] - cf[3]) * cf[4] * cf[6]);
        } else {
            r[j] = u[j] * (z[j] > 0.0f ? 1.0f : lds_cf[0]);
        }
    }
    return r;
}

// SG_DZ_SHUFFLE: packed columns 8 q + 4 h .. + 3 of the stage's convolution at its pixel (y, x) of image n; H, W: the stage's input.
__device__ __forceinline__ d_f32x4 sg_dz4_shuffle(const SrgDz& s, float slope, size_t n, int q, int h, int y, int x, int H, int W) {
    const int co = 4 * (q >> 1);
    const size_t off = (((n * 8 + co / 8) * (size_t)(2 * H) + (2 * y + (q & 1))) * (size_t)(2 * W) + (2 * x + h)) * 8 + (co & 7);
    d_f32x4 u = *reinterpret_cast<const d_f32x4*>(s.up + off);
    const d_f32x4 v = *reinterpret_cast<const d_f32x4*>(s.z + off);
#pragma unroll
    for (int j = 0; j < 4; ++j) u[j] *= v[j] > 0.0f ? 1.0f : slope;
    return u;
}

// ---------------------------------------------------------------------------------------------------------------------------
// BatchNorm / PReLU sums.  k_disc_bn_bwd_part's thread layout for 64 channels, three sums per channel.
struct SrgBnPartArgs {
    SrgDz dz;             // BN: coef is unused (the sums come first), st and mi give y and xh
    const float* st;      // BN: (scale, shift) pairs
    const double* mi;     // BN: (mean, invstd) pairs
    const float* slope;   // the PReLU after this tensor, or null: none
    double* slab;         // slab[(c*3 + k)*rows + row], k = 0: sum g, 1: sum g*xh, 2: sum of up*y over y <= 0; row = image * strips + strip
    long long rows, P;
    int strips, n0;
};

template <int DZ>
__global__ void __launch_bounds__(D_THREADS) k_srg_bn_part(const SrgBnPartArgs a) {
    static_assert(DZ == SG_DZ_BN || DZ == SG_DZ_PRELU, "a tensor with an activation");
    constexpr int PS = D_THREADS / 16;   // pixel slots
    __shared__ double red[D_THREADS * 12];
    const int tid = threadIdx.x, half = tid & 1, ps = (tid >> 1) % PS, cb = tid / (2 * PS);
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const long long p0 = (long long)blockIdx.x * D_BN_STRIP;
    const long long p1 = p0 + D_BN_STRIP < a.P ? p0 + D_BN_STRIP : a.P;
    const size_t base = ((n * 8 + cb) * (size_t)a.P) * 8 + half * 4;
    const bool act = a.slope != nullptr;
    const float slope = act ? a.slope[0] : 1.0f;
    float s[4], t[4], mean[4], inv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = cb * 8 + half * 4 + j;
        s[j] = DZ == SG_DZ_BN ? a.st[2 * c] : 1.0f;
        t[j] = DZ == SG_DZ_BN ? a.st[2 * c + 1] : 0.0f;
        mean[j] = DZ == SG_DZ_BN ? (float)a.mi[2 * c] : 0.0f;
        inv[j] = DZ == SG_DZ_BN ? (float)a.mi[2 * c + 1] : 0.0f;
    }
    double acc[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) acc[i] = 0.0;
    for (long long p = p0 + ps; p < p1; p += PS) {
        const d_f32x4 z = *reinterpret_cast<const d_f32x4*>(a.dz.z + base + (size_t)p * 8);
        const d_f32x4 u = *reinterpret_cast<const d_f32x4*>(a.dz.up + base + (size_t)p * 8);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float y = DZ == SG_DZ_BN ? d_bn(s[j], z[j], t[j]) : z[j];
            const bool pos = y > 0.0f;
            const float g = u[j] * (pos ? 1.0f : slope);
            const float xh = (z[j] - mean[j]) * inv[j];
            acc[3 * j] += (double)g;
            acc[3 * j + 1] += (double)g * (double)xh;
            if (act && !pos) acc[3 * j + 2] += (double)u[j] * (double)y;
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) red[tid * 12 + i] = acc[i];
    __syncthreads();
    if (tid < 64) {
        const int cb2 = tid >> 3, h2 = (tid & 7) >> 2, j = tid & 3;
        double r0 = 0.0, r1 = 0.0, r2 = 0.0;
        for (int q = 0; q < PS; ++q) {
            const int src = ((cb2 * PS + q) * 2 + h2) * 12 + 3 * j;
            r0 += red[src];
            r1 += red[src + 1];
            r2 += red[src + 2];
        }
        const long long row = (long long)n * a.strips + blockIdx.x;
        a.slab[(size_t)(tid * 3) * a.rows + row] = r0;
        a.slab[(size_t)(tid * 3 + 1) * a.rows + row] = r1;
        a.slab[(size_t)(tid * 3 + 2) * a.rows + row] = r2;
    }
}

struct SrgBnRedArgs {
    const double* slab;
    long long rows;
    double count;          // N * H * W
    const float* gamma;    // null: a PReLU without a BatchNorm (head, upscale stage): only `chan` is written
    const float* st;
    const double* mi;
    const float* slope;    // the PReLU after this BatchNorm, or null
    float* coef;           // out [64][D_COEF]
    float* dgamma;         // out [64], may be null
    float* dbeta;          // out [64], may be null
    double* chan;          // out [64]: the channel's share of the slope gradient
};

__global__ void __launch_bounds__(D_THREADS) k_srg_bn_reduce(const SrgBnRedArgs a) {
    __shared__ double r[3][D_THREADS];
    const int c = blockIdx.x, tid = threadIdx.x;
    const double* p = a.slab + (size_t)(c * 3) * a.rows;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (long long i = tid; i < a.rows; i += D_THREADS) {
        s0 += p[i];
        s1 += p[a.rows + i];
        s2 += p[2 * a.rows + i];
    }
    r[0][tid] = s0;
    r[1][tid] = s1;
    r[2][tid] = s2;
    __syncthreads();
    for (int off = D_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) {
            r[0][tid] += r[0][tid + off];
            r[1][tid] += r[1][tid + off];
            r[2][tid] += r[2][tid + off];
        }
        __syncthreads();
    }
    if (tid == 0) {
        a.chan[c] = r[2][0];
        if (a.gamma) {
            const double dbeta = r[0][0], dgamma = r[1][0];
            const double mean = a.mi[2 * c], inv = a.mi[2 * c + 1];
            float* cf = a.coef + c * D_COEF;
            cf[0] = a.st[2 * c];
            cf[1] = a.st[2 * c + 1];
            cf[2] = (float)((double)a.gamma[c] * inv);
            cf[3] = (float)mean;
            cf[4] = (float)inv;
            cf[5] = (float)(dbeta / a.count);
            cf[6] = (float)(dgamma / a.count);
            cf[7] = a.slope ? a.slope[0] : 1.0f;
            if (a.dgamma) a.dgamma[c] = (float)dgamma;
            if (a.dbeta) a.dbeta[c] = (float)dbeta;
        }
    }
}

// dst[b] = sum of src[b*rows .. b*rows + rows), one workgroup per b, fixed order.
__global__ void __launch_bounds__(D_THREADS) k_srg_sum(const double* src, long long rows, float* dst) {
    __shared__ double r[D_THREADS];
    const int tid = threadIdx.x;
    const double* p = src + (size_t)blockIdx.x * rows;
    double s = 0.0;
    for (long long i = tid; i < rows; i += D_THREADS) s += p[i];
    r[tid] = s;
    __syncthreads();
    for (int off = D_THREADS / 2; off > 0; off >>= 1) {
        if (tid < off) r[tid] += r[tid + off];
        __syncthreads();
    }
    if (tid == 0) dst[blockIdx.x] = (float)r[0];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Data gradient of a 3x3 convolution, stride 1, pad 1, 64 input channels: k_disc_dgrad<CD, 64, 1>'s tile and loops.
struct SrgDgradArgs {
    SrgDz dz;
    const float* w;       // CD = 64: the trunk segment's packed weights [8][9 taps][8][64]; CD = 256: k_sr_up's [2][8][9][8][128]
    float* out;           // C8, 64 channels, H x W
    const float* add;     // a second gradient of the same tensor, added to the result; or null
    int H, W;             // the convolution's input (SHUFFLE: `up` and `z` are 2H x 2W)
    int tiles_x;
    int n0;
};

template <int CD, int DZ>
__global__ void __launch_bounds__(D_THREADS, 2) k_srg_dgrad(const SrgDgradArgs a) {
    static_assert((CD == 256) == (DZ == SG_DZ_SHUFFLE) && (CD == 64 || CD == 256), "a trunk convolution or an upscale stage");
    using G = DiscDgradGeom<CD, 64, 1>;
    constexpr int TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];
    __shared__ float lds_cf[DZ == SG_DZ_BN ? 64 * D_COEF : 1];

    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int i0 = ty * TH, j0 = tx * D_TW;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const size_t plane = (size_t)a.H * a.W;

    if (DZ == SG_DZ_BN)
        for (int i = tid; i < 64 * D_COEF; i += D_THREADS) lds_cf[i] = a.dz.coef[i];
    else if (DZ != SG_DZ_PLAIN && tid == 0)
        lds_cf[0] = a.dz.coef[0];

    d_f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * 4) * HWD + l16;
    const int wb = kq * WSTR + l16;

    for (int chunk = 0; chunk < G::CHUNKS; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk (and lds_cf is visible before the first one)
        // ---- dz halo of this chunk: global -> dz -> LDS planes
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int oy = i0 - 1 + hy, ox = j0 - 1 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (oy >= 0 && oy < a.H && ox >= 0 && ox < a.W) {
                    if constexpr (DZ == SG_DZ_SHUFFLE)
                        v = sg_dz4_shuffle(a.dz, lds_cf[0], n, chunk, h, oy, ox, a.H, a.W);
                    else
                        v = sg_dz4<DZ>(a.dz, lds_cf, ((n * 8 + chunk) * plane + (size_t)oy * a.W + ox) * 8 + h * 4, chunk * 8 + h * 4);
                }
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights, transposed: row (tap, dz channel) holds the 64 input channels
        for (int i = tid; i < 18 * 64; i += D_THREADS) {
            const int ci = i % 64, r = i / 64, h = r & 1, tap = r >> 1;
            const size_t row = (size_t)((ci >> 3) * 9 + tap) * 8 + (ci & 7);
            d_f32x4 v;
            if constexpr (CD == 64) {
                v = *reinterpret_cast<const d_f32x4*>(a.w + row * 64 + chunk * 8 + h * 4);
            } else {
                const int J = chunk * 8 + h * 4;
                v = *reinterpret_cast<const d_f32x4*>(a.w + (size_t)(J / 128) * (64 * 9 * 128) + row * 128 + J % 128);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_w[(tap * 8 + h * 4 + j) * WSTR + ci] = v[j];
        }
        __syncthreads();
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = 2 - tap / 3, dx = 2 - tap % 3;   // halo row / column of the tile's pixel (0, 0) for this tap
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

    const int ix = j0 + l16;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const int iy = i0 + wm * 4 + pt;
        if (iy < a.H && ix < a.W) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int ci = ct * 16 + kq * 4;
                const size_t at = (((n * 8 + ci / 8) * a.H + iy) * (size_t)a.W + ix) * 8 + (ci & 7);
                d_f32x4 v = acc[ct][pt];
                if (a.add) v = *reinterpret_cast<const d_f32x4*>(a.add + at) + v;
                *reinterpret_cast<d_f32x4*>(a.out + at) = v;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Weight and bias gradient of a 3x3 convolution, stride 1, pad 1, 64 input channels: k_disc_wgrad<64, 64, 1>'s items and loops.
struct SrgWgradArgs {
    SrgDz dz;
    const float* ain;       // C8, 64 channels, H x W: the tensor the staging turns into the convolution's input
    const float* st_in;     // IN_BN, IN_BN_PRELU: (scale, shift) of the BatchNorm in front
    const float* slope_in;  // IN_PRELU, IN_BN_PRELU: the PReLU in front
    float* part;            // out: part[(((split*4 + block)*CD_TOTAL + co)*9 + tap)*16 + ci%16]
    double* part_b;         // out: part_b[split*CD_TOTAL + co] (written by channel block 0)
    long long items;        // N * tiles
    int splits;
    int H, W;
    int tiles_x, tiles;
};

// Known limit, open ("fp32 weight-gradient chains that grow with N"): a workgroup's whole range of items is one
// fp32 accumulation chain, as k_disc_wgrad's was before D_WG_CHUNK (disc_bwd_kernels.h); no test runs it at an N where that shows.
template <int DZ, int IN, int CD_TOTAL = 64>
__global__ void __launch_bounds__(D_THREADS, 2) k_srg_wgrad(const SrgWgradArgs a) {
    static_assert((CD_TOTAL == 256) == (DZ == SG_DZ_SHUFFLE) && DZ != SG_DZ_PRELU, "a trunk convolution or an upscale stage");
    using G = DiscWgradGeom<1>;
    constexpr int HH = G::HH, HWD = G::HWD, RS = G::RS, XSTR = G::XSTR, ZSTR = G::ZSTR;
    constexpr bool BN_IN = IN == SG_IN_BN || IN == SG_IN_BN_PRELU, ACT_IN = IN == SG_IN_PRELU || IN == SG_IN_BN_PRELU;
    __shared__ float lds_a[16 * XSTR];
    __shared__ float lds_z[64 * ZSTR];
    __shared__ float lds_cf[DZ == SG_DZ_BN ? 64 * D_COEF : 1];
    __shared__ float lds_st[BN_IN ? 32 : 1];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x, blk = blockIdx.y;
    const long long it0 = a.items * split / a.splits, it1 = a.items * (split + 1) / a.splits;
    const size_t plane = (size_t)a.H * a.W;
    const int co0 = (int)blockIdx.z * 64;   // first packed column of this part

    if (DZ == SG_DZ_BN)
        for (int i = tid; i < 64 * D_COEF; i += D_THREADS) lds_cf[i] = a.dz.coef[i];
    else if (DZ == SG_DZ_SHUFFLE && tid == 0)
        lds_cf[0] = a.dz.coef[0];
    if (BN_IN && tid < 32) lds_st[tid] = a.st_in[blk * 32 + tid];
    const float slope_in = ACT_IN ? a.slope_in[0] : 1.0f;

    d_f32x4 acc[9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap) acc[tap] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    double bsum = 0.0;

    const int zb = (wave * 16 + l16) * ZSTR + kq * D_TW;
    const int ab = l16 * XSTR + kq * RS;

    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.tiles);
        const int t = (int)(item - (long long)n * a.tiles), ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const int oy0 = ty * D_WG_TH, ox0 = tx * D_TW;
        __syncthreads();   // every wave is done with the previous item (and the tables are visible before the first one)
        // ---- dz tile: 64 channels x 4 x 16 pixels (0 outside the tensor)
        for (int idx = tid; idx < 64 * 16; idx += D_THREADS) {
            const int h = idx & 1, c = (idx >> 1) & 15, r = (idx >> 5) & 3, cb = idx >> 7;
            const int oy = oy0 + r, ox = ox0 + c;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (oy < a.H && ox < a.W) {
                if constexpr (DZ == SG_DZ_SHUFFLE)
                    v = sg_dz4_shuffle(a.dz, lds_cf[0], n, co0 / 8 + cb, h, oy, ox, a.H, a.W);
                else
                    v = sg_dz4<DZ>(a.dz, lds_cf, ((n * 8 + cb) * plane + (size_t)oy * a.W + ox) * 8 + h * 4, cb * 8 + h * 4);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_z[(cb * 8 + h * 4 + j) * ZSTR + r * D_TW + c] = v[j];
        }
        // ---- halo of the 16 input channels of this block (what the forward staged; 0 outside the image)
        for (int idx = tid; idx < HH * HWD * 4; idx += D_THREADS) {
            const int q = idx / (HH * HWD), p = idx - q * (HH * HWD), cb2 = q >> 1, h = q & 1;
            const int hy = p / HWD, hx = p - hy * HWD;
            const int iy = oy0 - 1 + hy, ix = ox0 - 1 + hx;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                v = *reinterpret_cast<const d_f32x4*>(a.ain + ((n * 8 + blk * 2 + cb2) * plane + (size_t)iy * a.W + ix) * 8 + h * 4);
                const int c = cb2 * 8 + h * 4;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    if (BN_IN) v[j] = d_bn(lds_st[2 * (c + j)], v[j], lds_st[2 * (c + j) + 1]);
                    if (ACT_IN) v[j] = e_prelu(v[j], slope_in);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_a[(cb2 * 8 + h * 4 + j) * XSTR + hy * RS + hx] = v[j];
        }
        __syncthreads();
        if (blk == 0 && tid < 64) {
            double s = 0.0;
            for (int i = 0; i < D_WG_TH * D_TW; ++i) s += (double)lds_z[tid * ZSTR + i];
            bsum += s;
        }
        // ---- 16 k-steps (columns) of four pixel rows: 9 MFMAs per step per wave
#pragma unroll 4
        for (int col = 0; col < D_TW; ++col) {
            const float av = lds_z[zb + col];
#pragma unroll
            for (int tap = 0; tap < 9; ++tap) {
                const float bv = lds_a[ab + (tap / 3) * RS + col + tap % 3];
                acc[tap] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[tap], 0, 0, 0);
            }
        }
    }

    // a lane holds dz channels 4*kq .. 4*kq+3 of its wave's row tile for input channel l16
    float* part = a.part + (((size_t)split * 4 + blk) * CD_TOTAL + co0) * 144;
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int co = wave * 16 + kq * 4 + e;
            part[((size_t)co * 9 + tap) * 16 + l16] = acc[tap][e];
        }
    if (blk == 0 && tid < 64) a.part_b[(size_t)split * CD_TOTAL + co0 + tid] = bsum;
}

// k_disc_wgrad_reduce for an upscale stage: packed column J -> convolution channel s_up_conv_channel(J).
struct SrgWgradReduceArgs {
    const float* part;
    const double* part_b;
    float* dw;      // out [256][64][3][3], may be null
    float* db;      // out [256], may be null
    int splits;
};

__global__ void __launch_bounds__(D_THREADS) k_srg_wgrad_reduce(const SrgWgradReduceArgs a) {
    const int o = blockIdx.x * D_THREADS + threadIdx.x;
    constexpr int nw = 256 * 64 * 9;
    if (o < nw) {
        if (!a.dw) return;
        const int tap = o % 9, ci = (o / 9) % 64, J = o / (9 * 64);
        const size_t stride = (size_t)4 * 256 * 144;
        const float* p = a.part + (((size_t)(ci >> 4) * 256 + J) * 9 + tap) * 16 + (ci & 15);
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += (double)p[k * stride];
        a.dw[((size_t)s_up_conv_channel(J) * 64 + ci) * 9 + tap] = (float)s;
    } else if (o < nw + 256) {
        if (!a.db) return;
        const int J = o - nw;
        double s = 0.0;
        for (int k = 0; k < a.splits; ++k) s += a.part_b[(size_t)k * 256 + J];
        a.db[s_up_conv_channel(J)] = (float)s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// final's data gradient: du[n, ci, y, x] = sum_{co, kh, kw} dpre[n, co, y+4-kh, x+4-kw] * W[co, ci, kh, kw], a 16 x 16 pixel tile and
// all 64 channels per workgroup.  K runs over (co, kh, kw') with kw' = 0 .. 11: three MFMA k-steps per (co, kh), the weights of
// kw' >= 9 being zero.
constexpr int SG_TD_HALO = 24, SG_TD_RS = 25, SG_TD_PLANE = SG_TD_HALO * SG_TD_RS;
constexpr int SG_TD_WSTR = 64 + 16;

struct SrgTailDgradArgs {
    const float* grad_out;   // fp32 [N,3,H,W]
    const float* out;        // the forward's result (unused with raw)
    const float* w;          // the tail's segment: [64 ci][9 kh][32: co*9 + kw]
    float* du;               // out: C8, 64 channels, H x W
    int H, W;
    int tiles_x;
    int raw;
    int n0;
};

__global__ void __launch_bounds__(D_THREADS, 2) k_srg_tail_dgrad(const SrgTailDgradArgs a) {
    __shared__ float lds_x[3 * SG_TD_PLANE];
    __shared__ float lds_w[108 * SG_TD_WSTR];
    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const int y0 = ty * 16, x0 = tx * D_TW;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const size_t plane = (size_t)a.H * a.W;

    // ---- d(pre) halo, rows y0-4 .. y0+19, columns x0-4 .. x0+19, 0 outside the image
    for (int idx = tid; idx < 3 * SG_TD_HALO * SG_TD_HALO; idx += D_THREADS) {
        const int co = idx / (SG_TD_HALO * SG_TD_HALO), p = idx - co * (SG_TD_HALO * SG_TD_HALO);
        const int hy = p / SG_TD_HALO, hx = p - hy * SG_TD_HALO;
        const int y = y0 - 4 + hy, x = x0 - 4 + hx;
        float v = 0.0f;
        if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
            const size_t at = (n * 3 + co) * plane + (size_t)y * a.W + x;
            v = sg_dpre(a.grad_out[at], a.raw ? 0.0f : a.out[at], a.raw);
        }
        lds_x[co * SG_TD_PLANE + hy * SG_TD_RS + hx] = v;
    }

    d_f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int co = 0; co < 3; ++co) {
        __syncthreads();   // every wave is done with the previous channel's weights (and the halo is visible before the first one)
        // ---- rows (kh, kw') of this output channel's weights, 64 input channels each
        for (int i = tid; i < 108 * 64; i += D_THREADS) {
            const int ci = i & 63, r = i >> 6, kh = r / 12, kw = r - kh * 12;
            lds_w[r * SG_TD_WSTR + ci] = kw < 9 ? a.w[(size_t)(ci * 9 + kh) * E_TAIL_WROW + co * 9 + kw] : 0.0f;
        }
        __syncthreads();
        const float* xp = lds_x + co * SG_TD_PLANE;
        for (int kh = 0; kh < 9; ++kh) {
#pragma unroll
            for (int g3 = 0; g3 < 3; ++g3) {
                const int kw = g3 * 4 + kq;
                const int kwr = kw < 9 ? kw : 8;   // the padded k read a valid position; their weights are 0
                float av[4], bv[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) av[ct] = lds_w[(kh * 12 + kw) * SG_TD_WSTR + ct * 16 + l16];
#pragma unroll
                for (int pt = 0; pt < 4; ++pt) bv[pt] = xp[(wm * 4 + pt + 8 - kh) * SG_TD_RS + l16 + 8 - kwr];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct)
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
            }
        }
    }

    const int x = x0 + l16;
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const int y = y0 + wm * 4 + pt;
        if (y < a.H && x < a.W) {
#pragma unroll
            for (int ct = 0; ct < 4; ++ct) {
                const int ci = ct * 16 + kq * 4;
                *reinterpret_cast<d_f32x4*>(a.du + (((n * 8 + ci / 8) * a.H + y) * (size_t)a.W + x) * 8 + (ci & 7)) = acc[ct][pt];
            }
        }
    }
}

// final's bias gradient: per-strip sums of d(pre); slab[co*rows + row], row = image * strips + strip.
struct SrgTailBiasArgs {
    const float* grad_out;
    const float* out;
    double* slab;
    long long rows, P;
    int strips, raw, n0;
};

__global__ void __launch_bounds__(D_THREADS) k_srg_tail_bias_part(const SrgTailBiasArgs a) {
    __shared__ double r[D_THREADS];
    const int tid = threadIdx.x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const long long p0 = (long long)blockIdx.x * D_BN_STRIP;
    const long long p1 = p0 + D_BN_STRIP < a.P ? p0 + D_BN_STRIP : a.P;
    for (int co = 0; co < 3; ++co) {
        double s = 0.0;
        for (long long p = p0 + tid; p < p1; p += D_THREADS) {
            const size_t at = (n * 3 + co) * (size_t)a.P + (size_t)p;
            s += (double)sg_dpre(a.grad_out[at], a.raw ? 0.0f : a.out[at], a.raw);
        }
        __syncthreads();
        r[tid] = s;
        __syncthreads();
        for (int off = D_THREADS / 2; off > 0; off >>= 1) {
            if (tid < off) r[tid] += r[tid + off];
            __syncthreads();
        }
        if (tid == 0) a.slab[(size_t)co * a.rows + (long long)n * a.strips + blockIdx.x] = r[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// The head's weight, bias gradient on the VALU in fp64 (k_disc_wgrad0 for K = 243): dW[c, (ci, kh, kw)] = sum_p dz[c, p] *
// x[ci, p + (kh-4, kw-4)], slot 243: sum_p dz[c, p] (the bias).  An item is a segment of SG_W9_PX pixels of one image row; thread =
// (channel c, a quarter of K = 244).
constexpr int SG_W9_PX = 32, SG_W9_K = 244, SG_W9_KG = 61;

struct SrgWgrad9Args {
    SrgDz dz;              // (v0, gradient of x0, slope)
    const void* img;       // the input, fp32 [N,3,H,W] or uint8 [N,H,W,3]
    double* part;          // out: part[(split*64 + c)*244 + k]
    long long items;       // N * H * segments
    int splits, segs;
    int H, W;
    int u8;
};

// UNIT_U8: a uint8 image is read as (float)u / 255.0f, the ESRGAN generator's head (k_esr_head), not as d_u8's Normalize(0.5, 0.5).
template <bool UNIT_U8 = false>
__global__ void __launch_bounds__(D_THREADS) k_srg_wgrad243(const SrgWgrad9Args a) {
    __shared__ float lds_d[SG_W9_PX * 64];        // [pixel][c]
    __shared__ float lds_p[SG_W9_PX * SG_W9_K];   // [pixel][k]
    const int tid = threadIdx.x, c = tid & 63, kg = tid >> 6;
    const size_t plane = (size_t)a.H * a.W;
    const long long it0 = a.items * blockIdx.x / a.splits, it1 = a.items * (blockIdx.x + 1) / a.splits;
    const float slope = a.dz.coef[0];
    double acc[SG_W9_KG];
#pragma unroll
    for (int j = 0; j < SG_W9_KG; ++j) acc[j] = 0.0;
    for (long long item = it0; item < it1; ++item) {
        const long long row = item / a.segs;
        const int seg = (int)(item - row * a.segs);
        const size_t n = (size_t)(row / a.H);
        const int y = (int)(row - (long long)n * a.H), x0 = seg * SG_W9_PX;
        __syncthreads();
        for (int idx = tid; idx < SG_W9_PX * 16; idx += D_THREADS) {
            const int h = idx & 1, px = (idx >> 1) & (SG_W9_PX - 1), cb = idx >> 6;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (x0 + px < a.W) v = sg_dz4<SG_DZ_PRELU>(a.dz, &slope, ((n * 8 + cb) * plane + (size_t)y * a.W + (x0 + px)) * 8 + h * 4, 0);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_d[px * 64 + cb * 8 + h * 4 + j] = v[j];
        }
        for (int idx = tid; idx < SG_W9_PX * SG_W9_K; idx += D_THREADS) {
            const int px = idx / SG_W9_K, k = idx - px * SG_W9_K;
            float v = 0.0f;
            if (x0 + px < a.W) {
                if (k == 243) {
                    v = 1.0f;
                } else {
                    const int c3 = k / 81, kh = (k / 9) % 9, kw = k % 9;
                    const int iy = y + kh - 4, ix = x0 + px + kw - 4;
                    if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) {
                        const size_t pix = (size_t)iy * a.W + ix;
                        if (a.u8) {
                            const unsigned char u = static_cast<const unsigned char*>(a.img)[(n * plane + pix) * 3 + c3];
                            v = UNIT_U8 ? (float)u / 255.0f : d_u8(u);
                        } else {
                            v = static_cast<const float*>(a.img)[(n * 3 + c3) * plane + pix];
                        }
                    }
                }
            }
            lds_p[idx] = v;
        }
        __syncthreads();
        for (int px = 0; px < SG_W9_PX; ++px) {
            const double d = (double)lds_d[px * 64 + c];
            const float* pk = lds_p + px * SG_W9_K + kg * SG_W9_KG;
#pragma unroll
            for (int j = 0; j < SG_W9_KG; ++j) acc[j] += d * (double)pk[j];
        }
    }
    double* part = a.part + ((size_t)blockIdx.x * 64 + c) * SG_W9_K + kg * SG_W9_KG;
#pragma unroll
    for (int j = 0; j < SG_W9_KG; ++j) part[j] = acc[j];
}

// final's weight gradient on the MFMA: dW[co, ci, kh, kw] = sum_q u[ci, q] * dpre[co, q + (4-kh, 4-kw)], u = final's activated input
// (t as it is, or PReLU of the last stage's saved pre-activation).  k_srg_wgrad's items (4 x 16 pixels q) and A operand (the u tile,
// 16 channels per wave); the B operand of accumulator (co, kh) is d(pre)'s halo read at column offset -kw for MFMA column kw, so that
// columns 9 .. 15 are computed and dropped.  Partials leave in part[(split*64 + ci)*244 + (co, kh, kw)], k_srg_wgrad243's layout.
constexpr int SG_TW_HR = D_WG_TH + 8, SG_TW_HC = D_TW + 8, SG_TW_RS = SG_TW_HC + 1, SG_TW_PLANE = SG_TW_HR * SG_TW_RS;

struct SrgTailWgradArgs {
    const float* u;          // C8, 64 channels, H x W: t, or the last stage's pre-activation
    const float* slope;      // PRELU_IN: that stage's slope
    const float* grad_out;   // fp32 [N,3,H,W]
    const float* out;        // the forward's result (unused with raw)
    double* part;
    long long items;         // N * tiles
    int splits;
    int H, W;
    int tiles_x, tiles;
    int raw;
};

// Known limit, open ("fp32 weight-gradient chains that grow with N"): a workgroup's whole range of items is one
// fp32 accumulation chain, as k_disc_wgrad's was before D_WG_CHUNK (disc_bwd_kernels.h); no test runs it at an N where that shows.
template <bool PRELU_IN>
__global__ void __launch_bounds__(D_THREADS, 2) k_srg_tail_wgrad(const SrgTailWgradArgs a) {
    constexpr int ZSTR = DiscWgradGeom<1>::ZSTR;
    __shared__ float lds_u[64 * ZSTR];
    __shared__ float lds_g[3 * SG_TW_PLANE];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int split = blockIdx.x;
    const long long it0 = a.items * split / a.splits, it1 = a.items * (split + 1) / a.splits;
    const size_t plane = (size_t)a.H * a.W;
    const float slope = PRELU_IN ? a.slope[0] : 1.0f;

    d_f32x4 acc[27];
#pragma unroll
    for (int j = 0; j < 27; ++j) acc[j] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int ub = (wave * 16 + l16) * ZSTR + kq * D_TW;
    const int gb = (kq + 8) * SG_TW_RS + 8 - (l16 < 9 ? l16 : 8);   // columns 9 .. 15 read a valid position and are dropped

    for (long long item = it0; item < it1; ++item) {
        const size_t n = (size_t)(item / a.tiles);
        const int t = (int)(item - (long long)n * a.tiles), ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
        const int oy0 = ty * D_WG_TH, ox0 = tx * D_TW;
        __syncthreads();   // every wave is done with the previous item
        // ---- u tile: 64 channels x 4 x 16 pixels (0 outside the tensor)
        for (int idx = tid; idx < 64 * 16; idx += D_THREADS) {
            const int h = idx & 1, c = (idx >> 1) & 15, r = (idx >> 5) & 3, cb = idx >> 7;
            const int oy = oy0 + r, ox = ox0 + c;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (oy < a.H && ox < a.W) {
                v = *reinterpret_cast<const d_f32x4*>(a.u + ((n * 8 + cb) * plane + (size_t)oy * a.W + ox) * 8 + h * 4);
                if (PRELU_IN) {
#pragma unroll
                    for (int j = 0; j < 4; ++j) v[j] = e_prelu(v[j], slope);
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_u[(cb * 8 + h * 4 + j) * ZSTR + r * D_TW + c] = v[j];
        }
        // ---- d(pre) halo: rows oy0-4 .. oy0+7, columns ox0-4 .. ox0+19 (0 outside the image)
        for (int idx = tid; idx < 3 * SG_TW_HR * SG_TW_HC; idx += D_THREADS) {
            const int co = idx / (SG_TW_HR * SG_TW_HC), p = idx - co * (SG_TW_HR * SG_TW_HC);
            const int hy = p / SG_TW_HC, hx = p - hy * SG_TW_HC;
            const int y = oy0 - 4 + hy, x = ox0 - 4 + hx;
            float v = 0.0f;
            if (y >= 0 && y < a.H && x >= 0 && x < a.W) {
                const size_t at = (n * 3 + co) * plane + (size_t)y * a.W + x;
                v = sg_dpre(a.grad_out[at], a.raw ? 0.0f : a.out[at], a.raw);
            }
            lds_g[co * SG_TW_PLANE + hy * SG_TW_RS + hx] = v;
        }
        __syncthreads();
        // ---- 16 k-steps (columns) of four pixel rows: 27 MFMAs per step per wave
#pragma unroll 2
        for (int col = 0; col < D_TW; ++col) {
            const float av = lds_u[ub + col];
#pragma unroll
            for (int j = 0; j < 27; ++j) {
                const float bv = lds_g[(j / 9) * SG_TW_PLANE + gb - (j % 9) * SG_TW_RS + col];
                acc[j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv, acc[j], 0, 0, 0);
            }
        }
    }
    // a lane holds input channels 4*kq .. 4*kq+3 of its wave's row tile for kw = l16
    if (l16 < 9) {
#pragma unroll
        for (int j = 0; j < 27; ++j)
#pragma unroll
            for (int e = 0; e < 4; ++e)
                a.part[((size_t)split * 64 + wave * 16 + kq * 4 + e) * SG_W9_K + j * 9 + l16] = (double)acc[j][e];
    }
}

struct SrgWgrad9ReduceArgs {
    const double* part;
    float* dw;     // head: [64][243]; final: [3][64][81]; may be null
    float* db;     // head: [64]; may be null
    int splits, head;
};

__global__ void __launch_bounds__(D_THREADS) k_srg_wgrad243_reduce(const SrgWgrad9ReduceArgs a) {
    const int o = blockIdx.x * D_THREADS + threadIdx.x;
    if (o >= 64 * SG_W9_K) return;
    const int c = o / SG_W9_K, k = o - c * SG_W9_K;
    float* dst;
    if (k == 243) dst = a.head && a.db ? a.db + c : nullptr;
    else if (!a.dw) dst = nullptr;
    else dst = a.head ? a.dw + c * 243 + k : a.dw + ((size_t)(k / 81) * 64 + c) * 81 + k % 81;
    if (!dst) return;
    double s = 0.0;
    for (int i = 0; i < a.splits; ++i) s += a.part[(size_t)i * 64 * SG_W9_K + o];
    *dst = (float)s;
}

// ---------------------------------------------------------------------------------------------------------------------------
// The forward's packed blob from the parameter tensors (reference layouts, device memory) and the BatchNorm running buffers: what
// cid_sr_set_weight + cid_sr_upload_weights build on the host (sr_pack, api/srgan.h), byte for byte, gaps (0) included.  Grid y is
// the segment: 0 head, 1 .. 11 the trunk convolutions (11: mid), 12 .. the upscale stages, the last one the tail.  The eval-mode
// fold of BatchNorm l is pack_bn_fold's fp64 arithmetic with its roundings spelt out (the host rounds mean * s before it subtracts).
constexpr int SG_PACK_HEAD = E_HEAD_K * 64 + 128, SG_PACK_CONV = E_CONV_W + 256, SG_PACK_UP = S_UP_W + 256 + 64, SG_PACK_TAIL = E_TAIL_W + 64;

struct SrgPackArgs {
    const float* head_w;
    const float* head_b;
    const float* head_slope;
    const float* conv_w[S_TRAIN_BNS + 1];   // res_blocks.i.{0,3}.weight at 2i, 2i+1; mid.weight
    const float* conv_b[S_TRAIN_BNS + 1];
    const float* slope[S_TRAIN_BNS / 2];
    const float* gamma[S_TRAIN_BNS];
    const float* beta[S_TRAIN_BNS];
    const float* mean[S_TRAIN_BNS];
    const float* var[S_TRAIN_BNS];
    double eps[S_TRAIN_BNS];
    const float* up_w[3];
    const float* up_b[3];
    const float* up_slope[3];
    const float* tail_w;
    const float* tail_b;
    float* blob;
    int stages;
};

__global__ void __launch_bounds__(D_THREADS) k_srg_pack(const SrgPackArgs a) {
    const int seg = blockIdx.y, r = blockIdx.x * D_THREADS + threadIdx.x;
    float v = 0.0f;
    if (seg == 0) {
        if (r >= SG_PACK_HEAD) return;
        if (r < E_HEAD_K * 64) v = a.head_w[(r % 64) * E_HEAD_K + r / 64];
        else if (r < E_HEAD_K * 64 + 64) v = a.head_b[r - E_HEAD_K * 64];
        else if (r == E_HEAD_K * 64 + 64) v = a.head_slope[0];
        a.blob[r] = v;
    } else if (seg <= S_TRAIN_BNS + 1) {
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
            if (l == S_TRAIN_BNS) {   // mid: the identity fold
                v = is_t ? 0.0f : 1.0f;
            } else {
                const double s = (double)a.gamma[l][ch] / sqrt((double)a.var[l][ch] + a.eps[l]);
                v = is_t ? (float)__dsub_rn((double)a.beta[l][ch], __dmul_rn((double)a.mean[l][ch], s)) : (float)s;
            }
        } else if (r == E_CONV_SLOPE && l < S_TRAIN_BNS && l % 2 == 0) {
            v = a.slope[l / 2][0];
        }
        a.blob[SG_PACK_HEAD + (size_t)l * SG_PACK_CONV + r] = v;
    } else if (seg <= S_TRAIN_BNS + 1 + a.stages) {
        if (r >= SG_PACK_UP) return;
        const int u = seg - (S_TRAIN_BNS + 2);
        if (r < S_UP_W) {
            const int half = r / (64 * 9 * 128), rr = r - half * (64 * 9 * 128);
            const int J = half * 128 + rr % 128, q = rr / 128, ci8 = q & 7, tap = (q >> 3) % 9, chunk = (q >> 3) / 9;
            v = a.up_w[u][((size_t)s_up_conv_channel(J) * 64 + chunk * 8 + ci8) * 9 + tap];
        } else if (r < S_UP_SLOPE) {
            v = a.up_b[u][s_up_conv_channel(r - S_UP_BIAS)];
        } else if (r == S_UP_SLOPE) {
            v = a.up_slope[u][0];
        }
        a.blob[SG_PACK_HEAD + (size_t)(S_TRAIN_BNS + 1) * SG_PACK_CONV + (size_t)u * SG_PACK_UP + r] = v;
    } else {
        if (r >= SG_PACK_TAIL) return;
        if (r < E_TAIL_W) {
            const int col = r % E_TAIL_WROW, q = r / E_TAIL_WROW, kh = q % 9, ci = q / 9;
            if (col < 27) v = a.tail_w[(((size_t)(col / 9) * 64 + ci) * 9 + kh) * 9 + col % 9];
        } else if (r < E_TAIL_W + 3) {
            v = a.tail_b[r - E_TAIL_W];
        }
        a.blob[SG_PACK_HEAD + (size_t)(S_TRAIN_BNS + 1) * SG_PACK_CONV + (size_t)a.stages * SG_PACK_UP + r] = v;
    }
}

}  // namespace cid
