// cgan_kernels.h — gfx950 device kernels of the server's CGANGenerator forward (cid_cg_forward, include/cid.h), reference
// backend/app.py:105-143, the label branch, eval mode, fp32.
//
//     z    = box_muller of two hash streams, fp32 [N,100]                              k_cg_latent (when the caller draws it)
//     a0   = ReLU(BN0(l1(cat(z, label_emb[label])))) viewed as [N,128,8,8]             k_cg_linear
//     a_k  = ReLU(BN(ConvTranspose2d(CIN, COUT, 4, stride 2, padding 1)(a_{k-1})))     k_cg_up<CIN, COUT, HIN>, three times
//     out  = tanh(Conv2d(32, 3, 3, padding=1)(a_3))                                    k_cg_tail<OUT>
//
// Activations are fp32 in the C8 layout of disc_kernels.h.  Each BatchNorm arrives folded to y = fmaf(s, v, t) (cid_cg_upload_weights);
// ReLU is v < 0 ? 0 : v, which keeps a NaN.
//   * k_cg_linear: the 200 -> 8192 linear as a GEMM on v_mfma_f32_16x16x4_f32 with the features as MFMA rows and the IMAGES as
//     columns, so a column's sum never depends on the other columns.  One wave owns 16 features, keeps their 16 x 200 weights in
//     registers (each weight is read once per call) and walks the batch 16 images at a time, z's half of K and the embedding's half in
//     two accumulator chains that are added at the end.  The B operand is gathered on the fly:
//     k < 100 from z, k >= 100 from label_emb[label].  The 16 features of a tile are 4 channels x 4 pixels of the [128,8,8] view, so a
//     lane's four accumulators are four consecutive channels of one pixel and leave as one 16-byte store.  A label outside
//     [0, n_classes) reads row 0 and the image's outputs are replaced by NaN: nothing is indexed out of bounds.
//   * k_cg_up: out[oy] = sum in[iy] * w[ky] with oy = 2 iy - 1 + ky, so each output parity (py, px) = (oy & 1, ox & 1) is an ordinary
//     2 x 2 convolution of the input: output (2m + py, 2n + px) takes inputs (m - 1 + py + dy, n - 1 + px + dx), dy, dx in {0, 1},
//     with kernel taps (3 - py - 2 dy, 3 - px - 2 dx).  A 256-thread workgroup owns 8 rows x HIN columns of INPUT positions of one
//     image and all COUT channels; wave p computes parity p.  The input tile with its one-pixel halo is staged once per 4-channel
//     chunk and read by all four parities (their 16 taps are the 9 shifts of a 3 x 3 window); the chunk's 16 x 4 x COUT weights, packed
//     per parity at upload, sit beside it in LDS.  The next chunk is fetched into registers while the MFMAs of this one run.  Weights
//     are the A operand: a lane's four accumulators are four consecutive output channels of one output pixel, one 16-byte store.
//     Sizes are fixed by the model (8, 16, 32 are multiples of the 8-row tile), so there are no partial tiles.
//   * k_cg_tail<OUT>: Conv2d(32, 3, 3, padding=1) on the VALU, one thread per pixel, with tanhf, the server's uint8 view, or the raw
//     sums in the epilogue.
// Every sum has a fixed order, an image's workgroups depend on nothing but the image, and nothing is atomic.  Offsets are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include "disc_kernels.h"
#include "hash_streams.h"

namespace cid {

constexpr int CG_LATENT = 100;            // latent_dim: hard-coded by the reference's view(-1, 100, 1, 1)
constexpr int CG_FEAT = 128 * 8 * 8;      // l1's outputs
constexpr uint64_t CG_Z_U1 = fnv1a64("cgan:z:u1"), CG_Z_U2 = fnv1a64("cgan:z:u2");

typedef __attribute__((address_space(4))) const float* CgConstF;

__device__ __forceinline__ float cg_relu(float v) { return v < 0.0f ? 0.0f : v; }

// ---------------------------------------------------------------------------------------------------------------------------
// Latent: z[i, e] = (float)box_muller(u1, u2), element e of the two streams under seed seed0 + i (cid_add_noise's convention).
struct CgLatentArgs {
    float* z;         // [N,100]
    long long count;  // N * 100
    uint64_t seed0;   // seed + first_index
};

__global__ void __launch_bounds__(D_THREADS) k_cg_latent(const CgLatentArgs a) {
    const long long idx = (long long)blockIdx.x * D_THREADS + threadIdx.x;
    if (idx >= a.count) return;
    const uint64_t i = (uint64_t)(idx / CG_LATENT), e = (uint64_t)(idx % CG_LATENT);
    const uint64_t s = a.seed0 + i;
    const uint64_t ba = splitmix64(s ^ CG_Z_U1), bb = splitmix64(s ^ CG_Z_U2);
    a.z[idx] = (float)box_muller(unit_double(splitmix64(ba + e)), unit_double(splitmix64(bb + e)));
}

// ---------------------------------------------------------------------------------------------------------------------------
// Linear: cat(z, label_emb[label]) (200) -> 8192, + bias, BN0, ReLU -> [N,128,8,8] in C8.
constexpr int CG_LIN_STEPS = 50;          // k-steps of 4
constexpr int CG_LIN_LSTR = 52;           // floats per lane in the packed weights (13 x 16 bytes)
constexpr int CG_LIN_TILES = CG_FEAT / 16;
constexpr int CG_LIN_W = CG_LIN_TILES * 64 * CG_LIN_LSTR;
// the linear's segment of the blob: weights [tile][lane][52], biases in packed row order, s[128], t[128]
constexpr int CG_LIN_BIAS = CG_LIN_W, CG_LIN_S = CG_LIN_W + CG_FEAT, CG_LIN_T = CG_LIN_S + 128, CG_LIN_SEG = CG_LIN_T + 128;

// Feature (row of l1.weight) held by MFMA row `row` (0 .. 15) of 16-row tile `tile`: tile = (channel group of 4, pixel group of 4),
// row = 4 * (pixel in group) + (channel in group).  Host and device use this one function.
__host__ __device__ constexpr int cg_lin_feature(int tile, int row) { return (4 * (tile / 16) + row % 4) * 64 + 4 * (tile % 16) + row / 4; }

struct CgLinearArgs {
    const float* z;           // [N,100]
    const long long* labels;  // [N]
    float* out;               // C8, 128 channels, 8 x 8
    const float* w;           // the linear's segment
    const float* emb;         // [n_classes,100]
    int N, n_classes;
};

__global__ void __launch_bounds__(64) k_cg_linear(const CgLinearArgs a) {
    const int lane = threadIdx.x, l16 = lane & 15, kq = lane >> 4;
    const int tile = blockIdx.x;
    float av[CG_LIN_LSTR];
    {
        const d_f32x4* src = reinterpret_cast<const d_f32x4*>(a.w + ((size_t)tile * 64 + lane) * CG_LIN_LSTR);
#pragma unroll
        for (int i = 0; i < CG_LIN_LSTR / 4; ++i) {
            const d_f32x4 v = src[i];
#pragma unroll
            for (int j = 0; j < 4; ++j) av[i * 4 + j] = v[j];
        }
    }
    const int c0 = 4 * (tile / 16), p = 4 * (tile % 16) + kq;   // this lane's four channels and its pixel
    const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(a.w + CG_LIN_BIAS + tile * 16 + kq * 4);
    const d_f32x4 s4 = *reinterpret_cast<const d_f32x4*>(a.w + CG_LIN_S + c0);
    const d_f32x4 t4 = *reinterpret_cast<const d_f32x4*>(a.w + CG_LIN_T + c0);
    const float nan = __builtin_nanf("");

    for (int i0 = 0; i0 < a.N; i0 += 16) {
        const int i = i0 + l16;
        const bool valid = i < a.N;
        const long long lab = valid ? a.labels[i] : 0;
        const bool lab_ok = lab >= 0 && lab < a.n_classes;
        // a column past the batch repeats image 0 (its loads stay in bounds, nothing is stored for it): columns never mix
        const float* zrow = a.z + (size_t)(valid ? i : 0) * CG_LATENT + kq;
        const float* erow = a.emb + (size_t)(lab_ok ? lab : 0) * CG_LATENT + kq;
        float zv[CG_LIN_STEPS / 2], ev[CG_LIN_STEPS / 2];
#pragma unroll
        for (int s = 0; s < CG_LIN_STEPS / 2; ++s) {
            zv[s] = zrow[4 * s];
            ev[s] = erow[4 * s];
        }
        // two chains, z's half of K and the embedding's, added at the end: a fixed order
        d_f32x4 acc = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f}, acc_e = acc;
#pragma unroll
        for (int s = 0; s < CG_LIN_STEPS / 2; ++s) {
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], zv[s], acc, 0, 0, 0);
            acc_e = __builtin_amdgcn_mfma_f32_16x16x4f32(av[CG_LIN_STEPS / 2 + s], ev[s], acc_e, 0, 0, 0);
        }
        acc += acc_e;
        if (valid) {
            d_f32x4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = lab_ok ? cg_relu(d_bn(s4[r], acc[r] + b4[r], t4[r])) : nan;
            *reinterpret_cast<d_f32x4*>(a.out + (((size_t)i * 16 + c0 / 8) * 64 + p) * 8 + (c0 & 7)) = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Upsampling stage: ConvTranspose2d(CIN, COUT, 4, stride 2, padding 1) + bias -> BatchNorm -> ReLU, HIN x HIN -> 2 HIN x 2 HIN.
template <int CIN, int COUT, int HIN>
struct CgUpGeom {
    static constexpr int TR = 8;                                 // input rows per tile
    static constexpr int TILES = HIN / TR;                       // tiles per image
    static constexpr int HWD = HIN + 2;                          // halo columns
    static constexpr int NPIX = (TR + 2) * HWD;                  // halo pixels
    static constexpr int XSTR = NPIX + ((16 - NPIX % 32) + 32) % 32;   // plane stride = 16 mod 32 (DiscGeom::XSTR)
    static constexpr int WSTR = COUT + 16;                       // weight row stride in LDS
    static constexpr int PT = TR * HIN / 16;                     // 16-pixel MFMA column tiles per wave
    static constexpr int CT = COUT / 16;                         // 16-channel MFMA row tiles per wave
    static constexpr int CHUNKS = CIN / 4;
    static constexpr int WROWS = 64;                             // weight rows per chunk: (parity 4, tap 4, channel 4)
    static constexpr int X_ITERS = (NPIX + D_THREADS - 1) / D_THREADS;
    static constexpr int W_ITERS = WROWS * COUT / 4 / D_THREADS;
    static constexpr int W_SEG = 16 * CIN * COUT;                // packed weights; then bias, s, t of COUT each
    static_assert(HIN % TR == 0 && (TR * HIN) % 16 == 0, "whole tiles");
    static_assert(PT * CT == 32, "32 accumulator tiles per wave");
    static_assert(CIN % 8 == 0 && COUT % 16 == 0 && (WROWS * COUT / 4) % D_THREADS == 0, "chunking");
};

// Packed weight index of reference element w[ci][co][ky][kx] ([CIN,COUT,4,4]): chunk ci / 4, parity (py, px) = ((ky + 1) & 1,
// (kx + 1) & 1), tap (dy, dx) = ((3 - py - ky) / 2, (3 - px - kx) / 2).  Host-side packing and the kernel's addressing share it.
__host__ __device__ constexpr size_t cg_up_windex(int COUT, int ci, int co, int ky, int kx) {
    const int py = (ky + 1) & 1, px = (kx + 1) & 1, dy = (3 - py - ky) / 2, dx = (3 - px - kx) / 2;
    return ((size_t)((ci / 4) * 16 + (py * 2 + px) * 4 + dy * 2 + dx) * 4 + ci % 4) * COUT + co;
}

struct CgUpArgs {
    const float* in;    // C8, CIN channels, HIN x HIN
    float* out;         // C8, COUT channels, 2 HIN x 2 HIN
    const float* w;     // the stage's segment
};

template <int CIN, int COUT, int HIN>
__global__ void __launch_bounds__(D_THREADS, 2) k_cg_up(const CgUpArgs a) {
    using G = CgUpGeom<CIN, COUT, HIN>;
    constexpr int TR = G::TR, HWD = G::HWD, NPIX = G::NPIX, XSTR = G::XSTR, WSTR = G::WSTR, PT = G::PT, CT = G::CT;
    __shared__ float lds_x[4 * XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[G::WROWS * WSTR];

    const int tid = threadIdx.x, lane = tid & 63, par = tid >> 6;   // wave = output parity
    const int py = par >> 1, px = par & 1;
    const int l16 = lane & 15, kq = lane >> 4;
    const size_t n = blockIdx.x / G::TILES;
    const int y0 = (int)(blockIdx.x % G::TILES) * TR;
    constexpr size_t plane = (size_t)HIN * HIN;

    d_f32x4 acc[CT][PT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // this lane's B operand bases: plane kq, the halo position of its pixel of every column tile, shifted by the parity
    int xb[PT];
#pragma unroll
    for (int pt = 0; pt < PT; ++pt) {
        const int q = pt * 16 + l16;
        xb[pt] = kq * XSTR + (q / HIN + py) * HWD + (q % HIN) + px;
    }
    const int wb = (par * 16 + kq) * WSTR + l16;   // this lane's A operand base: its parity's rows, row kq of a tap, its channel

    // where this thread's share of a chunk comes from
    int x_off[G::X_ITERS];       // float offset inside the chunk's plane, or -1: outside the image (zero)
#pragma unroll
    for (int it = 0; it < G::X_ITERS; ++it) {
        const int idx = it * D_THREADS + tid;
        const int hy = idx / HWD, hx = idx - hy * HWD;
        const int iy = y0 - 1 + hy, ix = hx - 1;
        x_off[it] = (idx < NPIX && iy >= 0 && iy < HIN && ix >= 0 && ix < HIN) ? (iy * HIN + ix) * 8 : -1;
    }
    d_f32x4 xr[G::X_ITERS], wr[G::W_ITERS];
    const auto fetch = [&](int chunk) {
        const float* src = a.in + ((n * (CIN / 8) + chunk / 2) * plane) * 8 + (chunk & 1) * 4;
#pragma unroll
        for (int it = 0; it < G::X_ITERS; ++it) {
            xr[it] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (x_off[it] >= 0) xr[it] = *reinterpret_cast<const d_f32x4*>(src + x_off[it]);
        }
        const float* wsrc = a.w + (size_t)chunk * G::WROWS * COUT;
#pragma unroll
        for (int it = 0; it < G::W_ITERS; ++it) wr[it] = *reinterpret_cast<const d_f32x4*>(wsrc + (size_t)(it * D_THREADS + tid) * 4);
    };

    fetch(0);
    for (int chunk = 0; chunk < G::CHUNKS; ++chunk) {
        __syncthreads();   // every wave is done with the previous chunk
#pragma unroll
        for (int it = 0; it < G::X_ITERS; ++it) {
            const int idx = it * D_THREADS + tid;
            if (idx < NPIX) {
#pragma unroll
                for (int j = 0; j < 4; ++j) lds_x[j * XSTR + idx] = xr[it][j];
            }
        }
#pragma unroll
        for (int it = 0; it < G::W_ITERS; ++it) {
            const int i = it * D_THREADS + tid;
            const int r = i / (COUT / 4), c4 = i - r * (COUT / 4);
            *reinterpret_cast<d_f32x4*>(&lds_w[r * WSTR + c4 * 4]) = wr[it];
        }
        __syncthreads();
        if (chunk + 1 < G::CHUNKS) fetch(chunk + 1);   // in flight while this chunk's MFMAs run
        // ---- this parity's 2 x 2 taps, one k-step of 4 channels each
#pragma unroll
        for (int tap = 0; tap < 4; ++tap) {
            const int dy = tap >> 1, dx = tap & 1;
            float av[CT], bv[PT];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) av[ct] = lds_w[wb + tap * 4 * WSTR + ct * 16];
#pragma unroll
            for (int pt = 0; pt < PT; ++pt) bv[pt] = lds_x[xb[pt] + dy * HWD + dx];
#pragma unroll
            for (int ct = 0; ct < CT; ++ct)
#pragma unroll
                for (int pt = 0; pt < PT; ++pt) acc[ct][pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[ct], bv[pt], acc[ct][pt], 0, 0, 0);
        }
    }

    // ---- epilogue: + bias, BatchNorm, ReLU; four consecutive channels of output pixel (2 y + py, 2 x + px) per store
    constexpr int HO = 2 * HIN;
    const float* bias = a.w + G::W_SEG;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
        const int co = ct * 16 + kq * 4;
        const d_f32x4 b4 = *reinterpret_cast<const d_f32x4*>(bias + co);
        const d_f32x4 s4 = *reinterpret_cast<const d_f32x4*>(bias + COUT + co);
        const d_f32x4 t4 = *reinterpret_cast<const d_f32x4*>(bias + 2 * COUT + co);
#pragma unroll
        for (int pt = 0; pt < PT; ++pt) {
            const int q = pt * 16 + l16;
            const int oy = 2 * (y0 + q / HIN) + py, ox = 2 * (q % HIN) + px;
            d_f32x4 y;
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = cg_relu(d_bn(s4[r], acc[ct][pt][r] + b4[r], t4[r]));
            *reinterpret_cast<d_f32x4*>(a.out + (((n * (COUT / 8) + co / 8) * HO + oy) * (size_t)HO + ox) * 8 + (co & 7)) = y;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Tail: Conv2d(32, 3, 3, padding=1) + bias over 64 x 64 -> tanh as fp32 [N,3,64,64], the server's uint8 view [N,64,64,3], or the sum.
enum { CG_OUT_F32 = 0, CG_OUT_U8 = 1, CG_OUT_RAW = 2 };
constexpr int CG_TAIL_W = 32 * 9 * 3;     // [ci][tap][co], then the 3 biases
constexpr int CG_TAIL_SEG = 896;

struct CgTailArgs {
    const float* in;    // C8, 32 channels, 64 x 64
    void* out;
    const float* w;     // the tail's segment
    long long count;    // N * 4096
};

template <int OUT>
__global__ void __launch_bounds__(D_THREADS) k_cg_tail(const CgTailArgs a) {
    const long long gid = (long long)blockIdx.x * D_THREADS + threadIdx.x;
    if (gid >= a.count) return;
    const size_t n = (size_t)(gid >> 12);
    const int p = (int)(gid & 4095), y = p >> 6, x = p & 63;
    const CgConstF wc = (CgConstF)a.w;
    float acc[3];
#pragma unroll
    for (int co = 0; co < 3; ++co) acc[co] = wc[CG_TAIL_W + co];
    for (int cb = 0; cb < 4; ++cb) {
        const float* src = a.in + ((n * 4 + cb) * 4096) * 8;
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int iy = y + tap / 3 - 1, ix = x + tap % 3 - 1;
            d_f32x4 lo = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f}, hi = lo;
            if (iy >= 0 && iy < 64 && ix >= 0 && ix < 64) {
                const d_f32x4* s = reinterpret_cast<const d_f32x4*>(src + (size_t)(iy * 64 + ix) * 8);
                lo = s[0];
                hi = s[1];
            }
            const CgConstF wk = wc + (cb * 8 * 9 + tap) * 3;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float v = j < 4 ? lo[j & 3] : hi[j & 3];
#pragma unroll
                for (int co = 0; co < 3; ++co) acc[co] = fmaf(wk[j * 27 + co], v, acc[co]);
            }
        }
    }
#pragma unroll
    for (int co = 0; co < 3; ++co) {
        if (OUT == CG_OUT_U8) {   // y * 0.5 + 0.5 -> clamp(0, 1) -> mul(255).byte(): k_sr_tail's view arithmetic; NaN -> 0
            const float v = fminf(fmaxf(tanhf(acc[co]) * 0.5f + 0.5f, 0.f), 1.f);
            static_cast<unsigned char*>(a.out)[(n * 4096 + p) * 3 + co] = (unsigned char)(v * 255.0f);
        } else {
            static_cast<float*>(a.out)[(n * 3 + co) * 4096 + p] = OUT == CG_OUT_RAW ? acc[co] : tanhf(acc[co]);
        }
    }
}

}  // namespace cid
