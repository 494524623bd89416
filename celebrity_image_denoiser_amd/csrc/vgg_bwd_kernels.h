// vgg_bwd_kernels.h — gfx950 device kernels of the input gradient of the VGG content loss (cid_vgg_content_backward; the definition
// is in the header comment of include/cid.h).  The weights are frozen: there is no weight gradient, and none for operand b.
//
// The saved forward (cid_vgg_content_loss_saved) left the seven activations of both towers in the arena, fp32 C8, 2 N images each.
// The backward runs over the N images of tower a only; its gradient tensors are fp32 C8 with N images.
//   * k_vgg_seed: D3_3 = grad_out[n] * 2 / count * (f_a - f_b) where relu3_3(a) > 0, else 0; formed in double, rounded once.
//   * k_vgg_dgrad<CG, CX, UNPOOL, MASK, XPOS>: the data gradient of Conv2d(CX, CG, 3, pad 1), which is a 3x3 pad-1 convolution of
//     the CG-channel gradient with the flipped, transposed weights, as the batch-as-one-column-sequence implicit GEMM of
//     k_lpips_conv (lpips_kernels.h) on v_mfma_f32_16x16x4_f32: the same 128-column x 64-channel workgroup tile, the same LDS planes
//     (stride 16 mod 64) and weight rows, the same summation (MFMA chains in (chunk, kh, kw) order, cut every lp_flush(3) chunks, the
//     partial sums added in order).  The body is a copy: the forward's instantiations compile to what they did.
//       UNPOOL: the gradient operand is the gradient of a 2x2 / stride-2 max-pool's OUTPUT (half size); the max-pool's backward and
//       the ReLU mask of the pooled activation are taken while the operand is staged: position (y, x) gets the pooled gradient at
//       (y / 2, x / 2) if (y, x) is the first maximum of its window of the saved activation (ATen's rule: row-major, v > max ||
//       isnan(v)) and that activation is > 0, else zero; a row or column past 2 * floor(size / 2) gets zero.  No unpooled tensor exists.
//       MASK: the epilogue zeroes the result where the saved activation the gradient flows into is not > 0.
//   * k_vgg_head_bwd: Conv2d(3, 64, 3, pad 1) backward to the image on the VALU: one lane per pixel of the batch's pixel sequence,
//     three outputs, K = 576; the weights are wave-uniform scalar loads; per tap one chain over the 64 channels, the nine partial
//     sums added in tap order; x 0.5 under the unit view; fp32 NCHW.
// Every stored tensor is written exactly once.  Nothing is atomic; offsets are 64-bit.  A column's sum depends on the pixel's
// neighbourhood alone, never on the column slot, the batch size or the image's position.
#pragma once
#include <hip/hip_runtime.h>

#include "vgg_kernels.h"

namespace cid {

// ---------------------------------------------------------------------------------------------------------------------------
// Seed.  Thread t handles elements 4 t ... 4 t + 3 of tower a's relu3_3 in memory order.
struct VgSeedArgs {
    const float* tap;        // relu3_3: C8, 256 channels, 2 N images
    const double* grad_out;  // [N]
    float* out;              // D3_3: C8, 256 channels, N images
    long long count;         // 256 * H3 * W3 (a multiple of 4)
    long long total;         // N * count
    int N;
};

__global__ void __launch_bounds__(D_THREADS) k_vgg_seed(const VgSeedArgs a) {
    const long long i = ((long long)blockIdx.x * D_THREADS + threadIdx.x) * 4;
    if (i >= a.total) return;
    const long long n = i / a.count;
    const double scale = a.grad_out[n] * 2.0 / (double)a.count;
    const d_f32x4 u = *reinterpret_cast<const d_f32x4*>(a.tap + i);
    const d_f32x4 v = *reinterpret_cast<const d_f32x4*>(a.tap + (size_t)a.N * (size_t)a.count + i);
    d_f32x4 y;
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = u[e] > 0.0f ? (float)(scale * ((double)u[e] - (double)v[e])) : 0.0f;
    *reinterpret_cast<d_f32x4*>(a.out + i) = y;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Data gradient of a trunk convolution.  Packed weights: lp_conv_windex(CG, 3, cx, cg, kh, kw) holds w[cg][cx][2 - kh][2 - kw].
struct VgDgradArgs {
    const float* g;      // the gradient operand: C8, CG channels, N images; Ho x Wo, or with UNPOOL (Ho / 2) x (Wo / 2)
    const float* pool;   // UNPOOL: the saved activation that was pooled: C8, CG channels, Ho x Wo, tower a's N images first
    const float* act;    // MASK: the saved activation the result flows into: C8, CX channels, Ho x Wo, tower a's N images first
    float* out;          // C8, CX channels, Ho x Wo, N images
    const float* w;      // packed flipped, transposed weights
    long long total;     // N * Ho * Wo columns
    int Ho, Wo;
};

template <int CG, int CX, bool UNPOOL, bool MASK, int XPOS = LP_XPOS>
__global__ void __launch_bounds__(D_THREADS, 2) k_vgg_dgrad(const VgDgradArgs a) {
    constexpr int KS = 3, PAD = 1, TAPS = 9, CHUNKS = CG / 4, WROWS = TAPS * 4;
    constexpr int XSTR = XPOS + 16, X_ITERS = XPOS / D_THREADS;   // plane stride = 16 mod 64, as in k_lpips_conv
    static_assert(CG % 8 == 0 && CX % LP_MT == 0 && XPOS % 64 == 0 && XPOS % D_THREADS == 0, "channel blocks, bank offset");
    __shared__ float lds_x[4 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[WROWS * LP_WSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;       // this wave: channels 32 wm .. + 32, columns 64 wn .. + 64 of the workgroup's tile
    const int l16 = lane & 15, kq = lane >> 4;
    const int g = blockIdx.y;                      // channel group of the result
    const int Ho = a.Ho, Wo = a.Wo, P = Ho * Wo, WP = Wo + 2 * PAD;
    const int Hp = Ho / 2, Wp = Wo / 2;            // UNPOOL: the pooled map

    // ---- the run of columns and what it touches
    const long long q0 = (long long)blockIdx.x * LP_NT;
    const long long q_end = q0 + LP_NT < a.total ? q0 + LP_NT : a.total;
    const long long n_a = q0 / P, n_b = (q_end - 1) / P;
    const int ya = (int)(q0 - n_a * P) / Wo, yb = (int)((q_end - 1) - n_b * P) / Wo;
    const int S0 = ((n_a == n_b ? yb - ya + 1 : Ho - ya) + 2 * PAD) * WP;   // first image's region
    const int SM = (Ho + 2 * PAD) * WP;                                     // a whole image's
    const int npos = n_a == n_b ? S0 : S0 + (int)(n_b - n_a - 1) * SM + (yb + 1 + 2 * PAD) * WP;

    // where this thread's staged positions come from: float offset of (image, channel block 0, pixel) in the gradient operand, or -1
    // for zero (the halo; with UNPOOL also the row and column no window covers).  With UNPOOL p_off is the offset of the window's
    // first element in the pooled activation and p_me the position's own place in the window (2 * row + column).
    const size_t plane = (size_t)P * 8;
    const size_t gplane = UNPOOL ? (size_t)Hp * Wp * 8 : plane;
    long long x_off[X_ITERS];
    long long p_off[UNPOOL ? X_ITERS : 1];
    int p_me[UNPOOL ? X_ITERS : 1];
#pragma unroll
    for (int it = 0; it < X_ITERS; ++it) {
        const int idx = it * D_THREADS + tid;
        x_off[it] = -1;
        if (UNPOOL) p_off[it] = 0, p_me[it] = 0;
        if (idx < npos) {
            int j = 0, local = idx;
            if (idx >= S0) {
                j = 1 + (idx - S0) / SM;
                local = (idx - S0) - (j - 1) * SM;
            }
            const int r = local / WP, c = local - r * WP;
            const int iy = (j == 0 ? ya : 0) - PAD + r, ix = c - PAD;
            if (iy >= 0 && iy < Ho && ix >= 0 && ix < Wo) {
                if (UNPOOL) {
                    const int py = iy >> 1, px = ix >> 1;
                    if (py < Hp && px < Wp) {
                        x_off[it] = (long long)((size_t)(n_a + j) * (CG / 8) * gplane + ((size_t)py * Wp + px) * 8);
                        p_off[it] = (long long)((size_t)(n_a + j) * (CG / 8) * plane + ((size_t)(2 * py) * Wo + 2 * px) * 8);
                        p_me[it] = (iy & 1) * 2 + (ix & 1);
                    }
                } else {
                    x_off[it] = (long long)((size_t)(n_a + j) * (CG / 8) * plane + ((size_t)iy * Wo + ix) * 8);
                }
            }
        }
    }

    // this lane's B operand bases and output positions, one per column tile
    int xb[4];
    long long ob[4];   // (n * CX / 8) * P + p, or -1 past the end
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const long long q = q0 + wn * 64 + pt * 16 + l16;
        xb[pt] = kq * XSTR;
        ob[pt] = -1;
        if (q < a.total) {
            const long long n = q / P;
            const int p = (int)(q - n * P), y = p / Wo, x = p - y * Wo;
            const int j = (int)(n - n_a);
            xb[pt] += (j == 0 ? 0 : S0 + (j - 1) * SM) + (y - (j == 0 ? ya : 0)) * WP + x;
            ob[pt] = n * (CX / 8) * P + p;
        }
    }
    const int wb = kq * LP_WSTR + wm * 32 + l16;

    // two-level summation: `acc` is the MFMA chain of FLUSH chunks, `tot` the sum of those partial sums
    constexpr int FLUSH = lp_flush(KS);
    static_assert(CHUNKS % FLUSH == 0, "whole partial sums");
    d_f32x4 acc[2][4], tot[2][4];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = tot[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int chunk = 0; chunk < CHUNKS; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk
        const size_t coff = (size_t)(chunk >> 1) * gplane + (chunk & 1) * 4;
        const size_t poff = (size_t)(chunk >> 1) * plane + (chunk & 1) * 4;
#pragma unroll
        for (int it = 0; it < X_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < npos) {
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (x_off[it] >= 0) {
                    v = *reinterpret_cast<const d_f32x4*>(a.g + (size_t)x_off[it] + coff);
                    if (UNPOOL) {
                        const float* s = a.pool + (size_t)p_off[it] + poff;
                        d_f32x4 m = *reinterpret_cast<const d_f32x4*>(s);
                        int first[4] = {0, 0, 0, 0};
#pragma unroll
                        for (int t = 1; t < 4; ++t) {
                            const d_f32x4 u = *reinterpret_cast<const d_f32x4*>(s + ((size_t)(t >> 1) * Wo + (t & 1)) * 8);
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                if (u[e] > m[e] || u[e] != u[e]) {
                                    m[e] = u[e];
                                    first[e] = t;
                                }
                        }
                        // m is this position's own value wherever it is the window's first maximum
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = (first[e] == p_me[it] && m[e] > 0.0f) ? v[e] : 0.0f;
                    }
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) lds_x[e * XSTR + idx] = v[e];
            }
        }
        {
            const d_f32x4* wsrc = reinterpret_cast<const d_f32x4*>(a.w + ((size_t)g * CHUNKS + chunk) * WROWS * LP_MT);
            for (int i = tid; i < WROWS * (LP_MT / 4); i += D_THREADS) {
                const int r = i / (LP_MT / 4), c4 = i - r * (LP_MT / 4);
                *reinterpret_cast<d_f32x4*>(&lds_w[r * LP_WSTR + c4 * 4]) = wsrc[i];
            }
        }
        __syncthreads();
#pragma unroll
        for (int kh = 0; kh < KS; ++kh) {
#pragma unroll
            for (int kw = 0; kw < KS; ++kw) {
                const int toff = kh * WP + kw;
                float av[2], bv[4];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct) av[ct] = lds_w[wb + (kh * KS + kw) * 4 * LP_WSTR + ct * 16];
#pragma unroll
                for (int pt = 0; pt < 4; ++pt) bv[pt] = lds_x[xb[pt] + toff];
#pragma unroll
                for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
            }
        }
        if ((chunk + 1) % FLUSH == 0) {
#pragma unroll
            for (int ct = 0; ct < 2; ++ct)
#pragma unroll
                for (int pt = 0; pt < 4; ++pt) {
                    tot[ct][pt] += acc[ct][pt];
                    acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                }
        }
    }

    // ---- epilogue: the ReLU mask of the activation the gradient flows into; four consecutive channels of one pixel per store
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int co = g * LP_MT + wm * 32 + ct * 16 + kq * 4;
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            if (ob[pt] < 0) continue;
            const size_t at = ((size_t)ob[pt] + (size_t)(co / 8) * P) * 8 + (co & 7);
            d_f32x4 y = tot[ct][pt];
            if (MASK) {
                const d_f32x4 m = *reinterpret_cast<const d_f32x4*>(a.act + at);
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = m[r] > 0.0f ? y[r] : 0.0f;
            }
            *reinterpret_cast<d_f32x4*>(a.out + at) = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Head backward.  Weights: hb[(t * 64 + co) * 3 + ci] = w[co][ci][2 - t / 3][2 - t % 3]: tap t reads the gradient at
// (y - 1 + t / 3, x - 1 + t % 3).
constexpr int VG_HEADB_SEG = 9 * 64 * 3;

struct VgHeadBwdArgs {
    const float* g;      // D1_1: C8, 64 channels, H x W, N images
    float* out;          // grad_a: fp32 [N,3,H,W]
    const float* w;      // the head's backward segment
    long long total;     // N * H * W pixels
    int H, W;
    int unit;            // x 0.5: the derivative of v * 0.5 + 0.5
};

__global__ void __launch_bounds__(VG_HEAD_PIX) k_vgg_head_bwd(const VgHeadBwdArgs a) {
    const long long q = (long long)blockIdx.x * VG_HEAD_PIX + threadIdx.x;
    const bool valid = q < a.total;
    const long long qq = valid ? q : 0;
    const size_t HW = (size_t)a.H * a.W;
    const size_t n = (size_t)(qq / (long long)HW);
    const int p = (int)(qq - (long long)(n * HW));
    const int oy = p / a.W, ox = p - oy * a.W;
    const LpConstF wc = (LpConstF)a.w;

    float tot[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll 1   // one tap's 64 values in registers at a time
    for (int t = 0; t < 9; ++t) {
        const int iy = oy - 1 + t / 3, ix = ox - 1 + t % 3;
        const bool in = valid && iy >= 0 && iy < a.H && ix >= 0 && ix < a.W;
        const float* s = a.g + (n * 8 * HW + (size_t)(in ? iy * a.W + ix : 0)) * 8;
        d_f32x4 v[16];   // the tap's 64 channels first, so that their loads are in flight together
#pragma unroll
        for (int c4 = 0; c4 < 16; ++c4) {
            v[c4] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (in) v[c4] = *reinterpret_cast<const d_f32x4*>(s + (size_t)(c4 >> 1) * HW * 8 + (c4 & 1) * 4);
        }
        float part[3] = {0.0f, 0.0f, 0.0f};   // one tap's 64 products, then one addition into the running sum (see lp_flush)
#pragma unroll
        for (int c4 = 0; c4 < 16; ++c4)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const LpConstF wk = wc + (t * 64 + c4 * 4 + e) * 3;
#pragma unroll
                for (int ci = 0; ci < 3; ++ci) part[ci] = fmaf(wk[ci], v[c4][e], part[ci]);
            }
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) tot[ci] += part[ci];
    }
    if (valid) {
#pragma unroll
        for (int ci = 0; ci < 3; ++ci) a.out[(n * 3 + ci) * HW + p] = a.unit ? tot[ci] * 0.5f : tot[ci];
    }
}

}  // namespace cid
