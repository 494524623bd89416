// lpips_kernels.h — gfx950 device kernels of LPIPS(net='alex') (cid_lpips; the definition is in the header comment of include/cid.h).
//
// Both towers run as ONE batch of 2 N images: image n < N is operand a's image n, image N + n operand b's image n.  Activations are
// fp32 in the C8 layout of disc_kernels.h; the five taps stay in the workspace for the distance.
//   * k_lpips_head: operand read (fp32 [N,3,H,W] as it is, uint8 [N,H,W,3] through d_u8), the optional v*0.5+0.5, the scaling layer,
//     the 11x11 stride-4 convolution, bias and ReLU on the VALU.  A one-wave workgroup owns 64 output pixels and all 64 channels, so every
//     sample is read and scaled once; the K = 363 weight rows are wave-uniform and come through scalar loads, the sums stay in
//     registers, k order (ci, kh, kw), one partial sum per kernel row.
//   * k_lpips_conv<CIN, COUT, KS, POOL>: Conv2d(CIN, COUT, KS, padding KS/2) + bias + ReLU as an implicit GEMM on
//     v_mfma_f32_16x16x4_f32, weights as the A operand.  The GEMM's columns are the output pixels of the WHOLE batch in one sequence
//     (q = n * Ho * Wo + pixel), so a 16-column tile runs on over the end of an image into the next one and only the last tile of a
//     launch is partial, whatever the map's size (7 x 7, 1 x 1, ...).  A 256-thread workgroup owns LP_NT = 128 consecutive columns and
//     LP_MT = 64 channels (2 x 2 waves of 32 channels x 64 columns).  Per chunk of 4 input channels it stages (a) the rows of every
//     image its columns touch, with the zero halo, as 4 planes in LDS and (b) the chunk's KS x KS x 4 x 64 weights, which then serve
//     all 8 column tiles.  With POOL the staged value is the 3x3 / stride-2 maximum of the previous tap, taken during staging: no
//     pooled tensor exists.  A column's sum is MFMA chains in the order (chunk, kh, kw), cut every lp_flush(KS) chunks and added in order, with
//     the 4 channels of a chunk inside the MFMA: it depends on the pixel's neighbourhood alone, never on the column slot, the batch size or the image's position.
//   * k_lpips_dist: one workgroup per image pair, all five taps: per pixel the two channel norms, the weighted squared difference of
//     the unit vectors, then the pixel mean and the layer sum, everything in double in a fixed order (a tree over 256 partial sums).
// Nothing is atomic; offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include "disc_kernels.h"

namespace cid {

constexpr int LP_TAPS = 5;
__host__ __device__ constexpr int lp_channels(int k) { return k == 0 ? 64 : k == 1 ? 192 : k == 2 ? 384 : 256; }
__host__ __device__ constexpr int lp_lin_off(int k) { return k == 0 ? 0 : k == 1 ? 64 : k == 2 ? 256 : k == 3 ? 640 : 896; }
constexpr int LP_LIN_SEG = 1152;

typedef __attribute__((address_space(4))) const float* LpConstF;

__device__ __forceinline__ float lp_relu(float v) { return v < 0.0f ? 0.0f : v; }
// max that keeps a NaN, as ATen's max_pool2d does
__device__ __forceinline__ float lp_max(float m, float x) { return (x > m || x != x) ? x : m; }

// ---------------------------------------------------------------------------------------------------------------------------
// Head.  Segment: w[k][64] with k = (ci * 11 + kh) * 11 + kw, bias[64], shift[3] at LP_HEAD_SS, scale[3] at LP_HEAD_SS + 4.
constexpr int LP_HEAD_KS = 11, LP_HEAD_K = 3 * 11 * 11;
constexpr int LP_HEAD_B = LP_HEAD_K * 64, LP_HEAD_SS = LP_HEAD_B + 64, LP_HEAD_SEG = LP_HEAD_SS + 64;
constexpr int LP_HEAD_PIX = 64;   // output pixels per workgroup (one wave)

struct LpHeadArgs {
    const void* a;      // fp32 [N,3,H,W] or uint8 [N,H,W,3]
    const void* b;
    float* out;         // relu1: C8, 64 channels, H1 x W1, 2 N images
    const float* w;     // the head's segment
    int H, W, H1, W1;
    int N;              // images per tower
    int n0;             // first image (of 2 N) of this launch
    int u8a, u8b;       // operand formats
    int unit;           // v * 0.5 + 0.5 first
};

__global__ void __launch_bounds__(LP_HEAD_PIX) k_lpips_head(const LpHeadArgs a) {
    const int lane = threadIdx.x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int P1 = a.H1 * a.W1;
    const int p = (int)blockIdx.x * LP_HEAD_PIX + lane;
    const bool valid = p < P1;
    const int pp = valid ? p : 0;
    const int oy = pp / a.W1, ox = pp - oy * a.W1;
    const bool second = n >= (size_t)a.N;
    const void* src = second ? a.b : a.a;
    const bool u8 = second ? a.u8b != 0 : a.u8a != 0;
    const size_t img = second ? n - (size_t)a.N : n;
    const size_t HW = (size_t)a.H * a.W;
    const LpConstF wc = (LpConstF)a.w;

    float acc[64];
#pragma unroll
    for (int j = 0; j < 64; ++j) acc[j] = wc[LP_HEAD_B + j];
    for (int ci = 0; ci < 3; ++ci) {
        const float shift = wc[LP_HEAD_SS + ci], scale = wc[LP_HEAD_SS + 4 + ci];
        for (int kh = 0; kh < LP_HEAD_KS; ++kh) {
            const int iy = oy * 4 - 2 + kh;
            const bool row_in = iy >= 0 && iy < a.H;
            float part[64];   // one kernel row's 11 products, then one addition into the running sum (see lp_flush)
#pragma unroll
            for (int j = 0; j < 64; ++j) part[j] = 0.0f;
            float v[LP_HEAD_KS];   // the row's 11 samples first, so that their loads are in flight together
#pragma unroll
            for (int kw = 0; kw < LP_HEAD_KS; ++kw) {
                const int ix = ox * 4 - 2 + kw;
                v[kw] = 0.0f;   // the convolution's padding is zero AFTER the scaling layer
                if (row_in && ix >= 0 && ix < a.W) {
                    const size_t pix = (size_t)iy * a.W + ix;
                    if (u8) v[kw] = d_u8(static_cast<const unsigned char*>(src)[(img * HW + pix) * 3 + ci]);
                    else v[kw] = static_cast<const float*>(src)[(img * 3 + ci) * HW + pix];
                    if (a.unit) v[kw] = v[kw] * 0.5f + 0.5f;
                    v[kw] = (v[kw] - shift) / scale;
                }
            }
#pragma unroll
            for (int kw = 0; kw < LP_HEAD_KS; ++kw) {
                const LpConstF wk = wc + ((ci * LP_HEAD_KS + kh) * LP_HEAD_KS + kw) * 64;
#pragma unroll
                for (int j = 0; j < 64; ++j) part[j] = fmaf(wk[j], v[kw], part[j]);
            }
#pragma unroll
            for (int j = 0; j < 64; ++j) acc[j] += part[j];
        }
    }
    if (valid) {
#pragma unroll
        for (int cb = 0; cb < 8; ++cb) {
            float* dst = a.out + ((n * 8 + (size_t)cb) * P1 + p) * 8;
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                d_f32x4 y;
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = lp_relu(acc[cb * 8 + q * 4 + r]);
                *reinterpret_cast<d_f32x4*>(dst + q * 4) = y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// relu2 ... relu5.
constexpr int LP_NT = 128;                 // GEMM columns (output pixels of the batch sequence) per workgroup
constexpr int LP_MT = 64;                  // output channels per workgroup
constexpr int LP_XPOS = 2048;              // staged positions per plane, at most (the host checks lp_stage_bound against it)
constexpr int LP_WSTR = LP_MT + 16;        // weight row stride, 16 mod 64 likewise

// Positions a workgroup stages per plane: an upper bound over every run of LP_NT consecutive columns of maps Ho x Wo with halo `pad`.
// The first and the last image of a run are staged over the rows the run touches, the images between them whole; every staged row
// has Wo + 2 pad positions and every image 2 pad halo rows.
__host__ __device__ constexpr long long lp_stage_bound(int Ho, int Wo, int pad) {
    const long long P = (long long)Ho * Wo;
    const long long images = (LP_NT + P - 2) / P + 1;
    const long long rows_all = images * Ho, rows_run = LP_NT / Wo + 2 * images;
    return (images * 2 * pad + (rows_all < rows_run ? rows_all : rows_run)) * (Wo + 2 * pad);
}

// A column's K = CIN * KS * KS products are not summed in one chain: a single fp32 chain of 3,456 terms rounds at the running sum's
// magnitude every step, and the distances of near-identical images (differences of 1e-2 of the features) feel that.  The chain is cut
// every lp_flush(KS) chunks (100 - 144 products) and the partial sums are added in order: 12 - 24 roundings at full magnitude
// instead of up to 864.  The head does the same per kernel row.
__host__ __device__ constexpr int lp_flush(int KS) { return KS == 5 ? 1 : 4; }

// Packed index of w[co][ci][kh][kw] ([COUT,CIN,KS,KS]): channel group co / 64, chunk ci / 4, tap, ci % 4, co % 64.  Shared by the
// host-side packing and the kernel's addressing.
__host__ __device__ constexpr size_t lp_conv_windex(int CIN, int KS, int co, int ci, int kh, int kw) {
    return ((((size_t)(co / LP_MT) * (CIN / 4) + ci / 4) * (KS * KS) + kh * KS + kw) * 4 + ci % 4) * LP_MT + co % LP_MT;
}

struct LpConvArgs {
    const float* in;     // C8, CIN channels, Hs x Ws, 2 N images: the previous tap
    float* out;          // C8, COUT channels, Ho x Wo
    const float* w;      // packed weights, then COUT biases
    long long total;     // 2 N * Ho * Wo columns
    int Hs, Ws;          // the previous tap's size; with POOL, Ho = (Hs - PK) / 2 + 1, else Ho = Hs
    int Ho, Wo;
};

// PK is the pool's window (stride 2, no padding, floor mode): 3 for AlexNet, 2 for VGG (vgg_kernels.h).  XPOS is the plane size: a
// launch that stages more than LP_XPOS positions takes a wider plane (vgg_kernels.h).
template <int CIN, int COUT, int KS, bool POOL, int PK = 3, int XPOS = LP_XPOS>
__global__ void __launch_bounds__(D_THREADS, 2) k_lpips_conv(const LpConvArgs a) {
    constexpr int PAD = KS / 2, TAPS = KS * KS, CHUNKS = CIN / 4, WROWS = TAPS * 4;
    constexpr int XSTR = XPOS + 16, X_ITERS = XPOS / D_THREADS;   // plane stride = 16 mod 64: the 4 planes of a k-step sit 16 banks apart
    static_assert(CIN % 8 == 0 && COUT % LP_MT == 0 && XPOS % 64 == 0 && XPOS % D_THREADS == 0, "channel blocks, bank offset");
    __shared__ float lds_x[4 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[WROWS * LP_WSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;       // this wave: channels 32 wm .. + 32, columns 64 wn .. + 64 of the workgroup's tile
    const int l16 = lane & 15, kq = lane >> 4;
    const int g = blockIdx.y;                      // channel group
    const int Ho = a.Ho, Wo = a.Wo, P = Ho * Wo, WP = Wo + 2 * PAD;

    // ---- the run of columns and what it touches
    const long long q0 = (long long)blockIdx.x * LP_NT;
    const long long q_end = q0 + LP_NT < a.total ? q0 + LP_NT : a.total;
    const long long n_a = q0 / P, n_b = (q_end - 1) / P;
    const int ya = (int)(q0 - n_a * P) / Wo, yb = (int)((q_end - 1) - n_b * P) / Wo;
    const int S0 = ((n_a == n_b ? yb - ya + 1 : Ho - ya) + 2 * PAD) * WP;   // first image's region
    const int SM = (Ho + 2 * PAD) * WP;                                     // a whole image's
    const int npos = n_a == n_b ? S0 : S0 + (int)(n_b - n_a - 1) * SM + (yb + 1 + 2 * PAD) * WP;

    // where this thread's staged positions come from: float offset of (image, channel block 0, pixel), or -1 for the zero halo
    const size_t plane = (size_t)a.Hs * a.Ws * 8;
    long long x_off[X_ITERS];
#pragma unroll
    for (int it = 0; it < X_ITERS; ++it) {
        const int idx = it * D_THREADS + tid;
        x_off[it] = -1;
        if (idx < npos) {
            int j = 0, local = idx;
            if (idx >= S0) {
                j = 1 + (idx - S0) / SM;
                local = (idx - S0) - (j - 1) * SM;
            }
            const int r = local / WP, c = local - r * WP;
            const int iy = (j == 0 ? ya : 0) - PAD + r, ix = c - PAD;
            if (iy >= 0 && iy < Ho && ix >= 0 && ix < Wo) {
                const int sy = POOL ? 2 * iy : iy, sx = POOL ? 2 * ix : ix;
                x_off[it] = (long long)((size_t)(n_a + j) * (CIN / 8) * plane + ((size_t)sy * a.Ws + sx) * 8);
            }
        }
    }

    // this lane's B operand bases and output positions, one per column tile
    int xb[4];
    long long ob[4];   // (n * COUT / 8) * P + p, or -1 past the end
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
            ob[pt] = n * (COUT / 8) * P + p;
        }
    }
    const int wb = kq * LP_WSTR + wm * 32 + l16;

    // two-level summation: `acc` is the MFMA chain of LP_FLUSH chunks, `tot` the sum of those partial sums
    constexpr int FLUSH = lp_flush(KS);
    static_assert(CHUNKS % FLUSH == 0, "whole partial sums");
    d_f32x4 acc[2][4], tot[2][4];
#pragma unroll
    for (int ct = 0; ct < 2; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = tot[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    for (int chunk = 0; chunk < CHUNKS; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk
        const size_t coff = (size_t)(chunk >> 1) * plane + (chunk & 1) * 4;
#pragma unroll
        for (int it = 0; it < X_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < npos) {
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (x_off[it] >= 0) {
                    const float* s = a.in + (size_t)x_off[it] + coff;
                    v = *reinterpret_cast<const d_f32x4*>(s);
                    if (POOL) {
#pragma unroll
                        for (int t = 1; t < PK * PK; ++t) {
                            const d_f32x4 u = *reinterpret_cast<const d_f32x4*>(s + ((size_t)(t / PK) * a.Ws + t % PK) * 8);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] = lp_max(v[e], u[e]);
                        }
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

    // ---- epilogue: + bias, ReLU; four consecutive channels of one pixel per store
    const float* bias = a.w + (size_t)COUT * CIN * TAPS;
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int co = g * LP_MT + wm * 32 + ct * 16 + kq * 4;
        const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(bias + co);
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            if (ob[pt] < 0) continue;
            d_f32x4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = lp_relu(tot[ct][pt][r] + b4[r]);
            *reinterpret_cast<d_f32x4*>(a.out + ((size_t)ob[pt] + (size_t)(co / 8) * P) * 8 + (co & 7)) = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Distance: out[n] = sum_k mean_p sum_c w_k[c] (x0 / (|x0| + 1e-10) - x1 / (|x1| + 1e-10))^2, in double.
struct LpDistArgs {
    const float* tap[LP_TAPS];   // C8, 2 N images each
    const float* lin;            // the five lin weights, lp_lin_off
    double* out;                 // [N]
    double* layers;              // [N][5] or null
    int P[LP_TAPS];              // pixels per image of each tap
    int N;
};

struct LpAlexTaps {
    static __host__ __device__ constexpr int channels(int k) { return lp_channels(k); }
    static __host__ __device__ constexpr int lin_off(int k) { return lp_lin_off(k); }
};

// NET names the five taps' channel counts and where their lin weights start; the arithmetic is the same for every network.
template <class NET = LpAlexTaps>
__global__ void __launch_bounds__(D_THREADS) k_lpips_dist(const LpDistArgs a) {
    __shared__ double red[D_THREADS];
    const int tid = threadIdx.x;
    const size_t n = blockIdx.x;
    double total = 0.0;
#pragma unroll
    for (int k = 0; k < LP_TAPS; ++k) {
        const int CB = NET::channels(k) / 8, P = a.P[k];
        const float* x0 = a.tap[k] + n * CB * (size_t)P * 8;
        const float* x1 = a.tap[k] + (n + (size_t)a.N) * CB * (size_t)P * 8;
        const float* w = a.lin + NET::lin_off(k);
        double part = 0.0;
        for (int p = tid; p < P; p += D_THREADS) {
            double s0 = 0.0, s1 = 0.0;
            for (int cb = 0; cb < CB; ++cb) {
                const float* u0 = x0 + ((size_t)cb * P + p) * 8;
                const float* u1 = x1 + ((size_t)cb * P + p) * 8;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const d_f32x4 v0 = *reinterpret_cast<const d_f32x4*>(u0 + h * 4), v1 = *reinterpret_cast<const d_f32x4*>(u1 + h * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        s0 += (double)v0[e] * (double)v0[e];
                        s1 += (double)v1[e] * (double)v1[e];
                    }
                }
            }
            const double n0 = sqrt(s0) + 1e-10, n1 = sqrt(s1) + 1e-10;
            double d = 0.0;
            for (int cb = 0; cb < CB; ++cb) {
                const float* u0 = x0 + ((size_t)cb * P + p) * 8;
                const float* u1 = x1 + ((size_t)cb * P + p) * 8;
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const d_f32x4 v0 = *reinterpret_cast<const d_f32x4*>(u0 + h * 4), v1 = *reinterpret_cast<const d_f32x4*>(u1 + h * 4);
                    const d_f32x4 w4 = *reinterpret_cast<const d_f32x4*>(w + cb * 8 + h * 4);
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const double t = (double)v0[e] / n0 - (double)v1[e] / n1;
                        d += ((double)w4[e] * t) * t;
                    }
                }
            }
            part += d;
        }
        red[tid] = part;
        __syncthreads();
        for (int s = D_THREADS / 2; s > 0; s >>= 1) {
            if (tid < s) red[tid] += red[tid + s];
            __syncthreads();
        }
        const double dk = red[0] / (double)P;
        __syncthreads();   // red is rewritten by the next tap
        if (tid == 0 && a.layers) a.layers[n * LP_TAPS + k] = dk;
        total += dk;
    }
    if (tid == 0) a.out[n] = total;
}

}  // namespace cid
