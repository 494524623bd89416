// quality_kernels.h — gfx950 device kernels of the image-quality metrics (cid_quality, include/cid.h):
// PSNR, SSIM (7x7 box window) and MS-SSIM (11-tap Gaussian, five levels) of image pairs, the per-batch
// evaluation of the reference's denoise trainer (backend/trainingcode/denoise_gan_code/training.py:378-392).
//
// Bandwidth- and VALU-bound work, no matrix instructions:
//   * k_quality_tile: one 256-thread workgroup per (16x64-pixel tile, image) of one pyramid level.  Per channel it stages the
//     tile plus a halo (3 px for the box window, 5 px for the Gaussian) of both images in LDS, runs the horizontal pass of the five
//     moments (a, b, a^2, b^2, ab) into an LDS buffer and the vertical pass from it, evaluates the SSIM expression per pixel and
//     accumulates it in fp64 registers.  Moment maps never reach HBM.
//       - level 0 also sums (a-b)^2 for PSNR while it stages, so SSIM + PSNR read each input once, and runs MS-SSIM's level 0
//         on the same staged tile when it is requested;
//       - with POOL it writes the tile's share of the 2x2 average-pooled images of the next level (fp32 planes in the workspace).
//     Each workgroup writes its QSLOTS partial sums to its own slab row: no atomics.
//   * k_quality_finish: one wave per image reduces the image's slab rows in a fixed order in fp64 and applies log10 and the level
//     product.  An image's tiles depend only on (H, W), never on N, so its metrics are bit-identical in any batch.
#pragma once
#include <hip/hip_runtime.h>

namespace cid {

constexpr int Q_THREADS = 256;
constexpr int Q_TY = 16;     // owned rows per tile
constexpr int Q_TX = 64;     // owned columns per tile (one wave-width row)
constexpr int Q_LEVELS = 5;  // MS-SSIM levels
constexpr int QSLOTS = 10;   // partial sums per tile: box S [3], Gaussian cs [3], Gaussian ssim [3], sum (a-b)^2

// slab slot indices
constexpr int QS_BOX = 0, QS_CS = 3, QS_SS = 6, QS_D2 = 9;

struct QualityLevelArgs {
    const void* a;          // level 0: the caller's tensors (format fa / fb); levels >= 1: fp32 planes [N][3][H][W] in the workspace
    const void* b;
    int fa, fb;             // 0 = fp32 NCHW, 1 = uint8 NHWC (level 0 only)
    int H, W;               // this level's size
    int tiles_x;            // tiles per row of tiles (grid: x = tile, y = image n - n0)
    int n0;                 // first image of this launch
    float* pa;              // POOL: next level's planes [N][3][(H+1)/2][(W+1)/2]
    float* pb;
    double* part;           // slab rows of this level: part[(n * slab_stride + t) * QSLOTS + s]
    long long slab_stride;  // rows per image over all levels
    float g[11];            // Gaussian window (float32, normalised)
};

// One operand value as fp32.  u8 is ToTensor + Normalize(0.5,0.5) with true divisions, as k_conv_head and synth.normalize_u8.
__device__ __forceinline__ float q_load(const void* p, int fmt, size_t n, int c, int y, int x, int H, int W) {
    const size_t plane = (size_t)H * W, pix = (size_t)y * W + x;
    if (fmt == 1) {
        const unsigned char u = static_cast<const unsigned char*>(p)[(n * plane + pix) * 3 + c];
        return ((float)u / 255.0f - 0.5f) / 0.5f;
    }
    return static_cast<const float*>(p)[(n * 3 + c) * plane + pix];
}

// The two SSIM expressions are evaluated without FMA contraction: numerator and denominator then round alike, and SSIM(x, x) is 1.0
// exactly.
// skimage structural_similarity, one pixel: box means of the 7x7 window, sample covariance (49/48), data_range 2.
__device__ __forceinline__ float q_ssim_box(float sx, float sy, float sxx, float syy, float sxy) {
#pragma clang fp contract(off)
    const float inv = 1.0f / 49.0f, cn = 49.0f / 48.0f;
    const float C1 = (0.01f * 2.0f) * (0.01f * 2.0f), C2 = (0.03f * 2.0f) * (0.03f * 2.0f);
    const float ux = sx * inv, uy = sy * inv, uxx = sxx * inv, uyy = syy * inv, uxy = sxy * inv;
    const float vx = cn * (uxx - ux * ux), vy = cn * (uyy - uy * uy), vxy = cn * (uxy - ux * uy);
    return ((2.0f * (ux * uy) + C1) * (2.0f * vxy + C2)) / (((ux * ux + uy * uy) + C1) * ((vx + vy) + C2));
}
// pytorch_msssim _ssim, one pixel: Gaussian moments, compensation 1, data_range 1.  The moments are of the shifted images a - ka,
// b - kb (variances and covariance do not depend on the shift; the means get it back).  Returns cs; *ss = luminance * cs.
__device__ __forceinline__ float q_ssim_gauss(float dx, float dy, float gxx, float gyy, float gxy, float ka, float kb, float* ss) {
#pragma clang fp contract(off)
    const float C1 = 0.01f * 0.01f, C2 = 0.03f * 0.03f;
    const float vx = gxx - dx * dx, vy = gyy - dy * dy, vxy = gxy - dx * dy;
    const float mx = dx + ka, my = dy + kb;
    const float cs = (2.0f * vxy + C2) / ((vx + vy) + C2);
    *ss = ((2.0f * (mx * my) + C1) / ((mx * mx + my * my) + C1)) * cs;
    return cs;
}

// Horizontal pass of the five moments for rows [r0, r0 + rows) of the staged tile (taps K, centred), into hb[5][rows][Q_TX].
template <int K, int LW>
__device__ __forceinline__ void q_hpass(const float* sa, const float* sb, float* hb, int r0, int rows, int c0, const float* w) {
    for (int i = threadIdx.x; i < rows * Q_TX; i += Q_THREADS) {
        const int r = i / Q_TX, j = i % Q_TX;
        const float* pa = sa + (r0 + r) * LW + c0 + j;
        const float* pb = sb + (r0 + r) * LW + c0 + j;
        float m0 = 0.f, m1 = 0.f, m2 = 0.f, m3 = 0.f, m4 = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float x = pa[k], y = pb[k];
            const float wk = w ? w[k] : 1.0f;
            const float wx = wk * x, wy = wk * y;
            m0 += wx;
            m1 += wy;
            m2 = fmaf(wx, x, m2);
            m3 = fmaf(wy, y, m3);
            m4 = fmaf(wx, y, m4);
        }
        const int plane = rows * Q_TX;
        hb[i] = m0;
        hb[plane + i] = m1;
        hb[2 * plane + i] = m2;
        hb[3 * plane + i] = m3;
        hb[4 * plane + i] = m4;
    }
}

// Block-wide sum of QSLOTS doubles in a fixed order; thread 0 writes them to `dst`.
__device__ __forceinline__ void q_block_sum(double (&v)[QSLOTS], double* red, double* dst) {
#pragma unroll
    for (int s = 0; s < QSLOTS; ++s)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v[s] += __shfl_xor(v[s], off, 64);
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0)
#pragma unroll
        for (int s = 0; s < QSLOTS; ++s) red[wave * QSLOTS + s] = v[s];
    __syncthreads();
    if (threadIdx.x < QSLOTS) {
        double t = 0.0;
        for (int w = 0; w < Q_THREADS / 64; ++w) t += red[w * QSLOTS + threadIdx.x];
        dst[threadIdx.x] = t;
    }
}

// L0: level 0 (caller's tensors, values in [-1,1]; PSNR summed; the Gaussian pass reads x*0.5+0.5).  BOX: skimage SSIM.
// GAUSS: this level of MS-SSIM.  POOL: write the next level's pooled planes.
template <bool L0, bool BOX, bool GAUSS, bool POOL>
__global__ void __launch_bounds__(Q_THREADS) k_quality_tile(const QualityLevelArgs p) {
    constexpr int R = GAUSS ? 5 : 3;            // halo
    constexpr int LH = Q_TY + 2 * R, LW = Q_TX + 2 * R;
    constexpr int HB_ROWS = GAUSS ? Q_TY + 10 : Q_TY + 6;
    __shared__ float sa[LH * LW], sb[LH * LW];
    __shared__ float hb[(BOX || GAUSS) ? 5 * HB_ROWS * Q_TX : 1];
    __shared__ double red[(Q_THREADS / 64) * QSLOTS];

    const int H = p.H, W = p.W;
    const size_t n = (size_t)p.n0 + blockIdx.y;
    const int t = blockIdx.x;
    const int ty = t / p.tiles_x, tx = t - ty * p.tiles_x;
    const int y0 = ty * Q_TY, x0 = tx * Q_TX;

    double acc[QSLOTS];
#pragma unroll
    for (int s = 0; s < QSLOTS; ++s) acc[s] = 0.0;

#pragma unroll
    for (int c = 0; c < 3; ++c) {   // unrolled: acc[] is indexed by c and stays in registers
        // ---- stage tile + halo of both images; out-of-image words are 0 (never read by a valid output) ----
        for (int i = threadIdx.x; i < LH * LW; i += Q_THREADS) {
            const int r = i / LW, q = i % LW;
            const int y = y0 - R + r, x = x0 - R + q;
            float va = 0.f, vb = 0.f;
            if (y >= 0 && y < H && x >= 0 && x < W) {
                va = q_load(p.a, L0 ? p.fa : 0, n, c, y, x, H, W);
                vb = q_load(p.b, L0 ? p.fb : 0, n, c, y, x, H, W);
                if (L0 && r >= R && r < R + Q_TY && q >= R && q < R + Q_TX) {
                    const float d = va - vb;
                    acc[QS_D2] += (double)(d * d);
                }
            }
            sa[i] = va;
            sb[i] = vb;
        }
        __syncthreads();

        if constexpr (POOL) {
            // avg_pool2d(2, stride 2, padding (H%2, W%2), count_include_pad): output (py, px) averages rows 2py-ph, 2py-ph+1 and
            // columns 2px-pw, 2px-pw+1 (zeros outside).  This tile owns the outputs whose second row / column lies in it:
            // rows [y0/2, y0/2 + 8) x columns [x0/2, x0/2 + 32), one per thread.
            const int Hn = (H + 1) / 2, Wn = (W + 1) / 2, ph = H & 1, pw = W & 1;
            const int py = y0 / 2 + threadIdx.x / (Q_TX / 2), px = x0 / 2 + threadIdx.x % (Q_TX / 2);
            if (py < Hn && px < Wn) {
                float s0 = 0.f, s1 = 0.f;
#pragma unroll
                for (int dy = 0; dy < 2; ++dy)
#pragma unroll
                    for (int dx = 0; dx < 2; ++dx) {
                        const int y = 2 * py - ph + dy, x = 2 * px - pw + dx;
                        if (y >= 0 && x >= 0) {            // y < H and x < W hold by construction
                            const int li = (y - y0 + R) * LW + (x - x0 + R);
                            float va = sa[li], vb = sb[li];
                            if (L0) {
                                va = va * 0.5f + 0.5f;
                                vb = vb * 0.5f + 0.5f;
                            }
                            s0 += va;
                            s1 += vb;
                        }
                    }
                const size_t o = (n * 3 + c) * ((size_t)Hn * Wn) + (size_t)py * Wn + px;
                p.pa[o] = s0 / 4.0f;
                p.pb[o] = s1 / 4.0f;
            }
        }

        if constexpr (BOX) {
            q_hpass<7, LW>(sa, sb, hb, R - 3, Q_TY + 6, R - 3, nullptr);
            __syncthreads();
            constexpr int PL = (Q_TY + 6) * Q_TX;
            for (int i = threadIdx.x; i < Q_TY * Q_TX; i += Q_THREADS) {
                const int r = i / Q_TX, j = i % Q_TX;
                const int y = y0 + r, x = x0 + j;
                float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 7; ++k)
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] += hb[q * PL + (r + k) * Q_TX + j];
                if (y >= 3 && y < H - 3 && x >= 3 && x < W - 3) acc[QS_BOX + c] += (double)q_ssim_box(m[0], m[1], m[2], m[3], m[4]);
            }
            __syncthreads();
        }

        if constexpr (GAUSS) {
            float gw[11];
#pragma unroll
            for (int k = 0; k < 11; ++k) gw[k] = p.g[k];
            // E[x^2] - E[x]^2 in fp32 cancels badly for smooth images (C2 is 9e-4): the moments are taken of the tile shifted by
            // ka, kb = the mean of a 3x3 grid of its in-image pixels, which brings the window means near 0.  Level 0's input is
            // x*0.5+0.5 (rounded to fp32 as the definition says), applied in the same pass.
            __syncthreads();    // the pool above has read the unshifted tile
            float ka = 0.f, kb = 0.f;
            {
                const int hy = min(H - y0, Q_TY), hx = min(W - x0, Q_TX);
#pragma unroll
                for (int gy = 0; gy < 3; ++gy)
#pragma unroll
                    for (int gx = 0; gx < 3; ++gx) {
                        const int li = (R + (2 * gy + 1) * hy / 6) * LW + R + (2 * gx + 1) * hx / 6;
                        float va = sa[li], vb = sb[li];
                        if (L0) {
                            va = va * 0.5f + 0.5f;
                            vb = vb * 0.5f + 0.5f;
                        }
                        ka += va;
                        kb += vb;
                    }
                ka /= 9.0f;
                kb /= 9.0f;
            }
            __syncthreads();
            for (int i = threadIdx.x; i < LH * LW; i += Q_THREADS) {
                float va = sa[i], vb = sb[i];
                if (L0) {
                    va = va * 0.5f + 0.5f;
                    vb = vb * 0.5f + 0.5f;
                }
                sa[i] = va - ka;
                sb[i] = vb - kb;
            }
            __syncthreads();
            q_hpass<11, LW>(sa, sb, hb, 0, Q_TY + 10, 0, gw);
            __syncthreads();
            constexpr int PL = (Q_TY + 10) * Q_TX;
            for (int i = threadIdx.x; i < Q_TY * Q_TX; i += Q_THREADS) {
                const int r = i / Q_TX, j = i % Q_TX;
                const int y = y0 + r, x = x0 + j;
                float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 11; ++k)
#pragma unroll
                    for (int q = 0; q < 5; ++q) m[q] = fmaf(gw[k], hb[q * PL + (r + k) * Q_TX + j], m[q]);
                if (y >= 5 && y < H - 5 && x >= 5 && x < W - 5) {
                    float ss;
                    const float cs = q_ssim_gauss(m[0], m[1], m[2], m[3], m[4], ka, kb, &ss);
                    acc[QS_CS + c] += (double)cs;
                    acc[QS_SS + c] += (double)ss;
                }
            }
        }
        __syncthreads();    // the next channel overwrites sa / sb / hb
    }
    q_block_sum(acc, red, p.part + ((long long)n * p.slab_stride + t) * QSLOTS);
}

struct QualityFinishArgs {
    const double* part;      // slab [N][slab_stride][QSLOTS]
    long long slab_stride;
    int H, W;
    int level_tiles[Q_LEVELS];
    int level_off[Q_LEVELS]; // first slab row of each level
    int levels;              // 1 (PSNR / SSIM only) or 5 (MS-SSIM)
    int metrics;             // CID_METRIC_* bits
    int n0;                  // first image of this launch (grid: x = image n - n0)
    double* out;             // [N][3]
};

__device__ __forceinline__ double q_relu(double v) { return v > 0.0 ? v : (v != v ? v : 0.0); }   // torch.relu keeps NaN

// One wave per image: slab rows summed lane-strided then by a fixed butterfly, fp64 throughout.
__global__ void __launch_bounds__(64) k_quality_finish(const QualityFinishArgs p) {
    const size_t n = (size_t)p.n0 + blockIdx.x;
    const int lane = threadIdx.x;
    double tot[Q_LEVELS][QSLOTS] = {};
#pragma unroll
    for (int l = 0; l < Q_LEVELS; ++l) {
        if (l >= p.levels) break;
        double v[QSLOTS];
#pragma unroll
        for (int s = 0; s < QSLOTS; ++s) v[s] = 0.0;
        const double* base = p.part + ((long long)n * p.slab_stride + p.level_off[l]) * QSLOTS;
        for (int t = lane; t < p.level_tiles[l]; t += 64)
#pragma unroll
            for (int s = 0; s < QSLOTS; ++s) v[s] += base[(size_t)t * QSLOTS + s];
#pragma unroll
        for (int s = 0; s < QSLOTS; ++s) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v[s] += __shfl_xor(v[s], off, 64);
            tot[l][s] = v[s];
        }
    }
    if (lane != 0) return;
    const double qnan = __builtin_nan("");
    double psnr = qnan, ssim = qnan, msssim = qnan;
    const double H = p.H, W = p.W;
    if (p.metrics & 1) {
        const double mse = tot[0][QS_D2] / (3.0 * H * W);
        psnr = 10.0 * log10(4.0 / mse);               // mse == 0 -> +inf
    }
    if (p.metrics & 2) {
        const double cnt = (H - 6.0) * (W - 6.0);
        ssim = (tot[0][QS_BOX] / cnt + tot[0][QS_BOX + 1] / cnt + tot[0][QS_BOX + 2] / cnt) / 3.0;
    }
    if (p.metrics & 4) {
        const double wts[Q_LEVELS] = {0.0448, 0.2856, 0.3001, 0.2363, 0.1333};
        double sum = 0.0;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double v = 1.0;
            int h = p.H, w = p.W;
#pragma unroll
            for (int l = 0; l < Q_LEVELS; ++l) {
                const double cnt = (double)(h - 10) * (double)(w - 10);
                const double m = l < Q_LEVELS - 1 ? tot[l][QS_CS + c] / cnt : tot[l][QS_SS + c] / cnt;
                v *= pow(q_relu(m), wts[l]);
                h = (h + 1) / 2;
                w = (w + 1) / 2;
            }
            sum += v;
        }
        msssim = sum / 3.0;
    }
    p.out[n * 3 + 0] = psnr;
    p.out[n * 3 + 1] = ssim;
    p.out[n * 3 + 2] = msssim;
}

}  // namespace cid
