// srgan_kernels.h — gfx950 device kernels of the server's SRGANGenerator forward (cid_sr_forward, include/cid.h), reference
// backend/app.py:145-186, eval mode, fp32.
//
//     x0  = PReLU(Conv2d(3, 64, 9, pad 4)(x))                                        k_sr_head
//     r   = five blocks  b <- BN(Conv3x3(PReLU(BN(Conv3x3(b)))))   (no skip)          k_esr_conv<EPI_PRELU>, k_esr_conv<EPI_BN>
//     t   = Conv3x3(r) + x0                                                          k_esr_conv<EPI_RES>, (s, t) = (1, 0), res = x0
//     u  <- PReLU(PixelShuffle(2)(Conv2d(64, 256, 3, pad 1)(u)))   log2(scale) times  k_sr_up
//     out = tanh(Conv2d(64, 3, 9, pad 4)(u))                                         k_sr_tail<OUT>
//
// Activations are fp32 in the C8 layout of disc_kernels.h.  The trunk kernels are ESRGAN's (esrgan_kernels.h); new here:
//   * k_sr_head<U8>: k_esr_head's convolution with this model's input arithmetic.  fp32 [N,3,H,W] is taken as it is (already in
//     [-1,1]); uint8 [N,H,W,3] is read through d_u8, ToTensor + Normalize(0.5, 0.5) with true divisions.  The server's Pad(fill=0)
//     is index arithmetic: the network runs on Hp x Wp = (H + pt + pb) x (W + pl + pr), the band around the image reads as -1.0
//     (uint8 0 after Normalize) and positions outside the padded image as 0 (the convolution's own padding).
//   * k_sr_up: the 3x3 64 -> 256 convolution as an implicit GEMM on v_mfma_f32_16x16x4_f32 in the tiling of k_disc_conv<64, 128, 1>
//     (a 256-thread workgroup owns 8 x 16 input pixels and 128 of the 256 convolution channels; the two halves are grid z), with
//     bias, PixelShuffle(2) and the stage's PReLU in the epilogue.  The weight columns are packed so that MFMA row (kq, r) of the
//     g-th 16-row tile is convolution channel 4 * (4 g + r) + kq: a lane's four accumulators are then output channels 4 g .. 4 g + 3
//     of sub-pixel kq = 2 i + j and leave as one 16-byte store at output pixel (2 y + i, 2 x + j).  The 256-channel tensor never
//     exists in memory and the shuffle moves nothing between lanes.
//   * k_sr_tail<OUT>: k_esr_tail's sums (e_tail_sums) and tanhf, the server's uint8 view of it, or the raw sum.
// Every sum has a fixed order, an image's tiles depend only on the padded size, and nothing is atomic.  Offsets are 64-bit; a pixel
// index inside one image is an int (scale^2 * Hp * Wp < 2^31 is checked on the host).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "esrgan_kernels.h"

namespace cid {

// ---------------------------------------------------------------------------------------------------------------------------
// Head: Conv2d(3, 64, 9, padding=4) + bias + PReLU over the padded image -> x0 (C8, Hp x Wp).
struct SrHeadArgs {
    const void* in;     // fp32 [N,3,H,W] or uint8 [N,H,W,3]: the unpadded image
    float* x0;          // C8, Hp x Wp
    const float* w;     // k_esr_head's segment: [243 = (ci, kh, kw)][64 co], then the 64 biases, then the slope
    int H, W;           // the image
    int Hp, Wp;         // the padded image: H + pt + pb, W + pl + pr
    int pl, pt;         // where the image starts inside it
    int n0;
};

// SAVE (cid_sr_forward_saved): the sums before PReLU go to a.pre as well, x0's layout; the backward's masks and slope gradient need them.
struct SrHeadSavedArgs : SrHeadArgs {
    float* pre;
};

template <bool U8, bool SAVE = false>
__global__ void __launch_bounds__(D_THREADS) k_sr_head(const std::conditional_t<SAVE, SrHeadSavedArgs, SrHeadArgs> a) {
    const int p = blockIdx.x * D_THREADS + threadIdx.x;
    const long long HWp = (long long)a.Hp * a.Wp;
    if (p >= HWp) return;
    const size_t HW = (size_t)a.H * a.W;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int y = p / a.Wp, x = p - y * a.Wp;
    // Which of the window's 9 rows / columns lie in the padded image (`in`) and in the image itself (`img`), one bit each: decided
    // once per thread, so that the loops below carry no size or pad (the 64 wave-uniform weights of a tap need the scalar registers).
    unsigned rows_in = 0, rows_img = 0, cols_in = 0, cols_img = 0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int py = y + k - 4, px = x + k - 4;
        rows_in |= (unsigned)(py >= 0 && py < a.Hp) << k;
        rows_img |= (unsigned)(py - a.pt >= 0 && py - a.pt < a.H) << k;
        cols_in |= (unsigned)(px >= 0 && px < a.Wp) << k;
        cols_img |= (unsigned)(px - a.pl >= 0 && px - a.pl < a.W) << k;
    }
    const long long pix0 = (long long)(y - 4 - a.pt) * a.W + (x - 4 - a.pl);   // image pixel index of the window's corner (used where valid)
    const EsrConstF wc = (EsrConstF)a.w;
    float acc[64];
#pragma unroll
    for (int c = 0; c < 64; ++c) acc[c] = wc[E_HEAD_K * 64 + c];
    for (int ci = 0; ci < 3; ++ci)
        for (int kh = 0; kh < 9; ++kh) {
            const bool row_in = (rows_in >> kh) & 1, row_img = (rows_img >> kh) & 1;
            float v[9];
#pragma unroll
            for (int kw = 0; kw < 9; ++kw) {
                v[kw] = 0.0f;
                if (row_in && ((cols_in >> kw) & 1)) {
                    v[kw] = -1.0f;                // Pad(fill=0) -> ToTensor -> Normalize(0.5, 0.5)
                    if (row_img && ((cols_img >> kw) & 1)) {
                        const size_t pix = (size_t)(pix0 + (long long)kh * a.W + kw);
                        if (U8) v[kw] = d_u8(static_cast<const unsigned char*>(a.in)[(n * HW + pix) * 3 + ci]);
                        else v[kw] = static_cast<const float*>(a.in)[(n * 3 + ci) * HW + pix];
                    }
                }
            }
            const EsrConstF wk = wc + (ci * 9 + kh) * 9 * 64;
#pragma unroll
            for (int kw = 0; kw < 9; ++kw)
#pragma unroll
                for (int c = 0; c < 64; ++c) acc[c] = fmaf(wk[kw * 64 + c], v[kw], acc[c]);
        }
    const float slope = wc[E_HEAD_K * 64 + 64];
#pragma unroll
    for (int cb = 0; cb < 8; ++cb) {
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] = e_prelu(acc[cb * 8 + j], slope);
        d_f32x4* o = reinterpret_cast<d_f32x4*>(a.x0 + ((n * 8 + cb) * (size_t)HWp + p) * 8);
        o[0] = d_f32x4{v[0], v[1], v[2], v[3]};
        o[1] = d_f32x4{v[4], v[5], v[6], v[7]};
        if constexpr (SAVE) {
            d_f32x4* q = reinterpret_cast<d_f32x4*>(a.pre + ((n * 8 + cb) * (size_t)HWp + p) * 8);
            q[0] = d_f32x4{acc[cb * 8], acc[cb * 8 + 1], acc[cb * 8 + 2], acc[cb * 8 + 3]};
            q[1] = d_f32x4{acc[cb * 8 + 4], acc[cb * 8 + 5], acc[cb * 8 + 6], acc[cb * 8 + 7]};
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Upscale stage: Conv2d(64, 256, 3, padding=1) + bias -> PixelShuffle(2) -> PReLU, H x W -> 2H x 2W, 64 channels in and out.
constexpr int S_UP_W = 256 * 64 * 9;   // packed weights of one stage: [2 halves][8 chunks][9 taps][8][128 packed columns]
// one upscale segment of the blob: weights, then the 256 biases in packed column order, then the slope
constexpr int S_UP_BIAS = S_UP_W, S_UP_SLOPE = S_UP_W + 256;

// Packed column J (0 .. 255) of the stage's GEMM holds this convolution channel; J / 16 = g is the 16-row MFMA tile, whose rows
// (J % 16) = kq * 4 + r are sub-pixel kq of output channel 4 g + r.  Host and device use this one function.
__host__ __device__ constexpr int s_up_conv_channel(int J) { return 4 * (4 * (J / 16) + (J % 16) % 4) + (J % 16) / 4; }

struct SrUpArgs {
    const float* in;    // C8, 64 channels, H x W
    float* out;         // C8, 64 channels, 2H x 2W
    const float* w;     // the stage's segment
    int H, W;
    int tiles_x;
    int n0;
};

// SAVE (cid_sr_forward_saved): the shuffled sums before PReLU go to a.pre as well, out's layout.
struct SrUpSavedArgs : SrUpArgs {
    float* pre;
};

template <bool SAVE = false>
__global__ void __launch_bounds__(D_THREADS, 2) k_sr_up(const std::conditional_t<SAVE, SrUpSavedArgs, SrUpArgs> a) {
    using G = DiscGeom<64, 128, 1>;
    constexpr int WM = G::WM, TH = G::TH, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR;
    __shared__ float lds_x[8 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[72 * WSTR];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave % WM, wn = wave / WM;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int half = blockIdx.z;
    const int iy0 = ty * TH - 1, ix0 = tx * D_TW - 1;
    const size_t plane = (size_t)a.H * a.W;

    d_f32x4 acc[4][4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct)
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    const int xb = kq * XSTR + (wm * 4) * HWD + l16;   // this lane's B operand base (plane kq, its pixel column)
    const int wb = kq * WSTR + wn * 64 + l16;          // this lane's A operand base (row kq, its packed column)
    const float* whalf = a.w + (size_t)half * (64 * 9 * 128);

    for (int chunk = 0; chunk < 8; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk
        // ---- halo of this chunk: global -> VGPR -> LDS planes; outside the image: the convolution's zero padding
        const float* src = a.in + ((n * 8 + chunk) * plane) * 8;
#pragma unroll
        for (int it = 0; it < G::STAGE_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX * 2) {
                const int p = idx >> 1, h = idx & 1;
                const int hy = p / HWD, hx = p - hy * HWD;
                const int iy = iy0 + hy, ix = ix0 + hx;
                d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
                if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W)
                    v = *reinterpret_cast<const d_f32x4*>(src + ((size_t)iy * a.W + ix) * 8 + h * 4);
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * XSTR + p] = v[j];
            }
        }
        // ---- this chunk's weights: 72 rows (tap, channel) of this half's 128 packed columns
        const float* wsrc = whalf + (size_t)chunk * 72 * 128;
        for (int i = tid; i < 72 * 32; i += D_THREADS) {
            const int r = i >> 5, c4 = i & 31;
            *reinterpret_cast<d_f32x4*>(&lds_w[r * WSTR + c4 * 4]) = *reinterpret_cast<const d_f32x4*>(wsrc + r * 128 + c4 * 4);
        }
        __syncthreads();
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
                    for (int pt = 0; pt < 4; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
            }
        }
    }

    // ---- epilogue: + bias, PReLU, and the shuffle as an address: this lane holds sub-pixel kq of four consecutive output channels
    const int ix = tx * D_TW + l16;
    if (ix >= a.W) return;
    const float slope = a.w[S_UP_SLOPE];
    const int Ho = 2 * a.H, Wo = 2 * a.W;
    const int ox = 2 * ix + (kq & 1);
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const int g = half * 8 + wn * 4 + ct;          // the 16-row tile: output channels 4 g .. 4 g + 3
        const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(a.w + S_UP_BIAS + g * 16 + kq * 4);
        const int co = 4 * g;
#pragma unroll
        for (int pt = 0; pt < 4; ++pt) {
            const int iy = ty * TH + wm * 4 + pt;
            if (iy < a.H) {
                const int oy = 2 * iy + (kq >> 1);
                d_f32x4 y = acc[ct][pt] + b4;
                if constexpr (SAVE) *reinterpret_cast<d_f32x4*>(a.pre + (((n * 8 + co / 8) * Ho + oy) * (size_t)Wo + ox) * 8 + (co & 7)) = y;
#pragma unroll
                for (int r = 0; r < 4; ++r) y[r] = e_prelu(y[r], slope);
                *reinterpret_cast<d_f32x4*>(a.out + (((n * 8 + co / 8) * Ho + oy) * (size_t)Wo + ox) * 8 + (co & 7)) = y;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tail: tanh(Conv2d(64, 3, 9, padding=4) + bias) -> fp32 [N,3,H,W], the server's uint8 view [N,H,W,3], or the sum before tanh.
enum { SR_OUT_F32 = 0, SR_OUT_U8 = 1, SR_OUT_RAW = 2 };

template <int OUT>
__global__ void __launch_bounds__(E_TAIL_THREADS) k_sr_tail(const EsrTailArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[4 * E_TAIL_PLANE];
    const int tid = threadIdx.x;
    const int ry = tid >> 3, cx = (tid & 7) * E_TAIL_PX;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const size_t plane = (size_t)a.H * a.W;
    float acc[3][E_TAIL_PX];
    e_tail_sums(a, lds, ty, tx, n, acc);

    const int oy = ty * E_TAIL_TH + ry;
    if (oy >= a.H) return;
#pragma unroll
    for (int j = 0; j < E_TAIL_PX; ++j) {
        const int ox = tx * E_TAIL_TW + cx + j;
        if (ox < a.W) {
            const size_t pix = (size_t)oy * a.W + ox;
#pragma unroll
            for (int co = 0; co < 3; ++co) {
                if (OUT == SR_OUT_U8) {   // y * 0.5 + 0.5 -> clamp(0, 1) -> ToPILImage: the denoiser's view arithmetic (k_conv_tail)
                    const float v = fminf(fmaxf(tanhf(acc[co][j]) * 0.5f + 0.5f, 0.f), 1.f);
                    static_cast<unsigned char*>(a.out)[(n * plane + pix) * 3 + co] = (unsigned char)(v * 255.0f);
                } else {
                    static_cast<float*>(a.out)[(n * 3 + co) * plane + pix] = OUT == SR_OUT_RAW ? acc[co][j] : tanhf(acc[co][j]);
                }
            }
        }
    }
}

}  // namespace cid
