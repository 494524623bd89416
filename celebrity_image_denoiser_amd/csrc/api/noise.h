// Noise synthesis (cid_add_noise): argument checks and launches; kernels in noise_kernels.h.  Host code.
#pragma once
#include "../api_common.h"
#include "../noise_kernels.h"

namespace {

// exp(-lambda) for lambda = 0..255 from the host libm (std::exp), the value synth.add_poisson_noise takes from math.exp
const double* poisson_exp_table() {
    static double t[256];
    static const bool ready = [] {
        for (int l = 0; l < 256; ++l) t[l] = std::exp(-(double)l);
        return true;
    }();
    (void)ready;
    return t;
}

static_assert(CID_NOISE_GAUSSIAN == NK_GAUSSIAN && CID_NOISE_SALT_PEPPER == NK_SALT_PEPPER && CID_NOISE_SPECKLE == NK_SPECKLE &&
                  CID_NOISE_POISSON == NK_POISSON && CID_NOISE_UNIFORM == NK_UNIFORM, "noise kind enums out of sync");

}  // namespace

extern "C" {

int cid_add_noise(const void* clean_u8_nhwc, void* out_u8_nhwc, int N, int H, int W, int kind, const double* params, int nparams,
                  uint64_t seed, uint64_t first_index, void* stream) {
    if (!clean_u8_nhwc || !out_u8_nhwc) return CID_ERR_INVALID;
    if (kind < CID_NOISE_GAUSSIAN || kind > CID_NOISE_UNIFORM) return CID_ERR_INVALID;
    const int want = kind == CID_NOISE_POISSON ? 0 : 2;
    if (nparams != want || (want && !params)) return CID_ERR_INVALID;
    for (int i = 0; i < want; ++i)
        if (!std::isfinite(params[i])) return CID_ERR_INVALID;
    if ((kind == CID_NOISE_GAUSSIAN || kind == CID_NOISE_SPECKLE) && params[1] < 0.0) return CID_ERR_INVALID;
    if (kind == CID_NOISE_SALT_PEPPER && (params[0] < 0.0 || params[0] > 1.0 || params[1] < 0.0 || params[1] > 1.0))
        return CID_ERR_INVALID;
    if (kind == CID_NOISE_UNIFORM && params[0] > params[1]) return CID_ERR_INVALID;
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if (kind == CID_NOISE_SALT_PEPPER && (H < 2 || W < 2)) return CID_ERR_SHAPE;
    if ((long long)H * W * 3 >= 0x80000000LL) return CID_ERR_SHAPE;

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int per = H * W * 3;
    const uint64_t seed0 = seed + first_index;
    const unsigned gy = (unsigned)std::min(N, NOISE_MAX_GRID_Y);

    if (kind == CID_NOISE_SALT_PEPPER) {
        if (out_u8_nhwc != clean_u8_nhwc &&
            hipMemcpyAsync(out_u8_nhwc, clean_u8_nhwc, (size_t)N * per, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return CID_ERR_HIP;
        for (int pass = 0; pass < 2; ++pass) {   // salt, then pepper: stream order makes pepper win a collision
            NoiseScatterArgs a{};
            a.out = static_cast<uint8_t*>(out_u8_nhwc);
            a.N = N;
            a.H = H;
            a.W = W;
            a.draws = (int)((double)per * params[pass]);   // int(float(H*W*3) * prob); <= per
            a.seed0 = seed0;
            a.stream_row = pass ? NS_PEPPER_ROW : NS_SALT_ROW;
            a.stream_col = pass ? NS_PEPPER_COL : NS_SALT_COL;
            a.value = pass ? 0 : 255;
            if (a.draws == 0) continue;
            const dim3 grid((unsigned)((a.draws + NOISE_THREADS - 1) / NOISE_THREADS), gy);
            hipLaunchKernelGGL(k_noise_scatter, grid, dim3(NOISE_THREADS), 0, s, a);
            if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
        }
        return CID_OK;
    }

    NoiseArgs a{};
    a.in = static_cast<const uint8_t*>(clean_u8_nhwc);
    a.out = static_cast<uint8_t*>(out_u8_nhwc);
    a.N = N;
    a.per = per;
    a.seed0 = seed0;
    if (want) {
        a.p0 = params[0];
        a.p1 = params[1];
    }
    const dim3 grid((unsigned)((per + NOISE_THREADS * NOISE_EPT - 1) / (NOISE_THREADS * NOISE_EPT)), gy), block(NOISE_THREADS);
    switch (kind) {
        case CID_NOISE_GAUSSIAN:
            a.stream_a = NS_GAUSS_U1;
            a.stream_b = NS_GAUSS_U2;
            hipLaunchKernelGGL(k_noise_elem<NK_GAUSSIAN>, grid, block, 0, s, a);
            break;
        case CID_NOISE_SPECKLE:
            a.stream_a = NS_SPECKLE_U1;
            a.stream_b = NS_SPECKLE_U2;
            hipLaunchKernelGGL(k_noise_elem<NK_SPECKLE>, grid, block, 0, s, a);
            break;
        case CID_NOISE_UNIFORM:
            a.stream_a = NS_UNIFORM;
            hipLaunchKernelGGL(k_noise_elem<NK_UNIFORM>, grid, block, 0, s, a);
            break;
        default:   // CID_NOISE_POISSON
            a.stream_a = NS_POISSON;
            std::memcpy(a.exp_neg, poisson_exp_table(), sizeof a.exp_neg);
            hipLaunchKernelGGL(k_noise_elem<NK_POISSON>, grid, block, 0, s, a);
            break;
    }
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
