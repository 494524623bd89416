// noise_kernels.h — gfx950 device kernels of the noise synthesis (cid_add_noise, include/cid.h): the five noise kinds the
// reference's denoise trainer is trained on (backend/trainingcode/denoise_gan_code/noise_generation.py:6-39, training.py:247),
// applied to uint8 NHWC batches on the device.
//
// Every random draw comes from the counter-based splitmix64 streams of synth.py: image n of a launch uses the seed
// s = seed + first_index + n, and element e of stream `id` is z = splitmix64(splitmix64(s ^ id) + e), u = (z >> 11) * 2^-53.
// Element e is the flat HWC index (y*W + x)*3 + c of the image, so an image's noise depends only on (seed, its global index,
// its size), never on the batch.  synth.add_noise_np is the bit-defined restatement.
//
//   * k_noise_elem<KIND>: one thread per element (4 elements per thread, strided by the block for coalescing), 2-D grid
//     (element blocks of one image x image).  Gaussian / speckle: Box-Muller, three fp64 transcendentals per element; uniform:
//     one draw; poisson: inversion by sequential search, lambda+1 iterations on average, the wave running as long as its slowest
//     lane.  Each thread reads its input byte before it writes its output byte, so out == in works.
//   * k_noise_scatter: salt & pepper.  One thread per draw writes the 3 channels of one pixel.  The caller copies the clean batch
//     first (unless in place) and launches salt then pepper on the same stream, so pepper wins a collision; racing threads of one
//     launch write the same value.
//
// The float64 arithmetic is written in numpy's order with contraction off: hipcc would otherwise fuse img + sigma*z into an FMA
// and round differently from the restatement.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "hash_streams.h"

namespace cid {

constexpr int NOISE_THREADS = 256;
constexpr int NOISE_EPT = 4;              // elements per thread
constexpr int NOISE_MAX_GRID_Y = 65535;   // images per grid row; larger batches loop in the kernel
constexpr int NOISE_POISSON_KMAX = 1023;  // inversion cut-off (never reached for lambda <= 255 but by rounding)

enum NoiseKind { NK_GAUSSIAN = 0, NK_SALT_PEPPER = 1, NK_SPECKLE = 2, NK_POISSON = 3, NK_UNIFORM = 4 };

// stream ids: gaussian keeps synth.add_gaussian_noise's 1 and 2; the other kinds hash their names clear of them
constexpr uint64_t NS_GAUSS_U1 = 1, NS_GAUSS_U2 = 2;
constexpr uint64_t NS_SPECKLE_U1 = fnv1a64("noise:speckle:u1"), NS_SPECKLE_U2 = fnv1a64("noise:speckle:u2");
constexpr uint64_t NS_UNIFORM = fnv1a64("noise:uniform");
constexpr uint64_t NS_POISSON = fnv1a64("noise:poisson");
constexpr uint64_t NS_SALT_ROW = fnv1a64("noise:salt_pepper:salt_row"), NS_SALT_COL = fnv1a64("noise:salt_pepper:salt_col");
constexpr uint64_t NS_PEPPER_ROW = fnv1a64("noise:salt_pepper:pepper_row");
constexpr uint64_t NS_PEPPER_COL = fnv1a64("noise:salt_pepper:pepper_col");

struct NoiseArgs {
    const uint8_t* in;        // [N][per] clean images
    uint8_t* out;             // [N][per]; may equal in
    int N;                    // images of this call
    int per;                  // H*W*3 elements per image
    uint64_t seed0;           // seed + first_index: image n uses seed0 + n
    uint64_t stream_a;        // u (uniform, poisson) or u1 (gaussian, speckle)
    uint64_t stream_b;        // u2 (gaussian, speckle)
    double p0, p1;            // (mean, sigma) or (low, high)
    double exp_neg[256];      // poisson: exp(-lambda) for lambda = 0..255, from the host's libm
};

struct NoiseScatterArgs {
    uint8_t* out;             // [N][H*W*3]
    int N, H, W;
    int draws;                // per image
    uint64_t seed0;
    uint64_t stream_row, stream_col;
    uint8_t value;            // 255 salt, 0 pepper
};

// np.clip(v, 0, 255).astype(np.uint8): clip, then truncate toward zero
__device__ __forceinline__ uint8_t clip_u8(double v) {
    return (uint8_t)(v < 0.0 ? 0 : (v > 255.0 ? 255 : (int)v));
}

template <int KIND>
__device__ __forceinline__ uint8_t noise_element(const NoiseArgs& a, const double* exp_neg, uint8_t x, uint64_t ba, uint64_t bb,
                                                 uint64_t e) {
#pragma clang fp contract(off)
    const double img = (double)x;
    if constexpr (KIND == NK_GAUSSIAN || KIND == NK_SPECKLE) {
        const double z = box_muller(unit_double(splitmix64(ba + e)), unit_double(splitmix64(bb + e)));
        const double n = a.p0 + a.p1 * z;
        return clip_u8(KIND == NK_GAUSSIAN ? img + n : img + img * n);
    } else if constexpr (KIND == NK_UNIFORM) {
        const double u = unit_double(splitmix64(ba + e));
        return clip_u8(img + (a.p0 + (a.p1 - a.p0) * u));
    } else {   // NK_POISSON: k mod 256, as the reference's np.random.poisson(u8).astype(np.uint8) wraps
        const double u = unit_double(splitmix64(ba + e));
        double p = exp_neg[x], c = p;
        int k = 0;
        while (u >= c && k < NOISE_POISSON_KMAX) {
            ++k;
            p = (p * img) / (double)k;
            c = c + p;
        }
        return (uint8_t)(k & 255);
    }
}

template <int KIND>
__global__ void __launch_bounds__(NOISE_THREADS) k_noise_elem(NoiseArgs a) {
    __shared__ double exp_neg[KIND == NK_POISSON ? 256 : 1];
    if constexpr (KIND == NK_POISSON) {
        exp_neg[threadIdx.x] = a.exp_neg[threadIdx.x];   // NOISE_THREADS == 256
        __syncthreads();
    }
    const long long e0 = (long long)blockIdx.x * (NOISE_THREADS * NOISE_EPT) + threadIdx.x;   // per < 2^31, e0 + 1023 may not be
    for (int n = blockIdx.y; n < a.N; n += gridDim.y) {
        const uint64_t s = a.seed0 + (uint64_t)n;
        const uint64_t ba = splitmix64(s ^ a.stream_a), bb = splitmix64(s ^ a.stream_b);
        const size_t img = (size_t)n * (size_t)a.per;
        const uint8_t* src = a.in + img;
        uint8_t* dst = a.out + img;
#pragma unroll
        for (int j = 0; j < NOISE_EPT; ++j) {
            const long long e = e0 + j * NOISE_THREADS;
            if (e < a.per) dst[e] = noise_element<KIND>(a, exp_neg, src[e], ba, bb, (uint64_t)e);
        }
    }
}

// One salt (or pepper) draw per thread: row = floor(z_r*(H-1) / 2^64), col = floor(z_c*(W-1) / 2^64), so the last row and column
// are never hit (numpy's randint(0, H-1)); all three channels of the pixel get `value`.
__global__ void __launch_bounds__(NOISE_THREADS) k_noise_scatter(NoiseScatterArgs a) {
    const long long j = (long long)blockIdx.x * NOISE_THREADS + threadIdx.x;
    if (j >= a.draws) return;
    const size_t per = (size_t)a.H * a.W * 3;
    for (int n = blockIdx.y; n < a.N; n += gridDim.y) {
        const uint64_t s = a.seed0 + (uint64_t)n;
        const uint64_t zr = splitmix64(splitmix64(s ^ a.stream_row) + (uint64_t)j);
        const uint64_t zc = splitmix64(splitmix64(s ^ a.stream_col) + (uint64_t)j);
        const int row = (int)__umul64hi(zr, (uint64_t)(a.H - 1));
        const int col = (int)__umul64hi(zc, (uint64_t)(a.W - 1));
        uint8_t* px = a.out + (size_t)n * per + ((size_t)row * a.W + col) * 3;
        px[0] = a.value;
        px[1] = a.value;
        px[2] = a.value;
    }
}

}  // namespace cid
