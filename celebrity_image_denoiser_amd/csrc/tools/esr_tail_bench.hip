// esr_tail_bench — the ESRGAN tail (Conv2d(64, 3, 9, pad 4), K = 5184) on the VALU (k_esr_tail, the product kernel) next to a plain
// implicit GEMM on v_mfma_f32_16x16x4_f32 whose 16-row weight tile holds the 3 output channels (k_esr_tail_mfma, this file only).
// Same input and weights for both; prints the largest difference and the median time of 5 windows of 10 launches.
//     make -C celebrity_image_denoiser_amd/csrc tools/esr_tail_bench && tools/esr_tail_bench [N H W]
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../esrgan_kernels.h"

#define HIP_OK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

namespace cid {

struct EsrTailMfmaArgs {
    const float* in;    // C8, 64 channels
    float* out;         // fp32 [N,3,H,W]
    const float* w;     // [8 chunks][81 taps][8 channels][4: co 0..2, then 0], then the 3 biases
    int H, W, tiles_x, n0;
};

constexpr int TM_HW = 24, TM_NPIX = TM_HW * TM_HW, TM_XSTR = TM_NPIX + 16;   // halo of a 16 x 16 tile; plane stride 16 mod 32

__global__ void __launch_bounds__(D_THREADS, 2) k_esr_tail_mfma(const EsrTailMfmaArgs a) {
    __shared__ float lds_x[8 * TM_XSTR];
    __shared__ __attribute__((aligned(16))) float lds_w[81 * 8 * 4];
    const int tid = threadIdx.x, lane = tid & 63, wm = tid >> 6;
    const int l16 = lane & 15, kq = lane >> 4;
    const int t = blockIdx.x, ty = t / a.tiles_x, tx = t - ty * a.tiles_x;
    const size_t n = (size_t)a.n0 + blockIdx.y;
    const int iy0 = ty * 16 - 4, ix0 = tx * 16 - 4;
    const size_t plane = (size_t)a.H * a.W;
    d_f32x4 acc[4];
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) acc[pt] = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const int xb = kq * TM_XSTR + (wm * 4) * TM_HW + l16;
    const int wb = kq * 4 + (l16 < 3 ? l16 : 3);   // rows 3..15 of the weight tile are zero
    for (int chunk = 0; chunk < 8; ++chunk) {
        __syncthreads();
        const float* src = a.in + ((n * 8 + chunk) * plane) * 8;
        for (int idx = tid; idx < TM_NPIX * 2; idx += D_THREADS) {
            const int p = idx >> 1, h = idx & 1;
            const int hy = p / TM_HW, hx = p - hy * TM_HW;
            const int iy = iy0 + hy, ix = ix0 + hx;
            d_f32x4 v = d_f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (iy >= 0 && iy < a.H && ix >= 0 && ix < a.W) v = *reinterpret_cast<const d_f32x4*>(src + ((size_t)iy * a.W + ix) * 8 + h * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) lds_x[(h * 4 + j) * TM_XSTR + p] = v[j];
        }
        const float* wsrc = a.w + (size_t)chunk * 81 * 8 * 4;
        for (int i = tid; i < 81 * 8; i += D_THREADS)
            *reinterpret_cast<d_f32x4*>(&lds_w[i * 4]) = *reinterpret_cast<const d_f32x4*>(wsrc + i * 4);
        __syncthreads();
#pragma unroll 1
        for (int kh = 0; kh < 9; ++kh)
#pragma unroll
            for (int kw = 0; kw < 9; ++kw)
#pragma unroll
                for (int sub = 0; sub < 2; ++sub) {
                    const float av = lds_w[wb + ((kh * 9 + kw) * 8 + sub * 4) * 4];
                    float bv[4];
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) bv[pt] = lds_x[xb + sub * 4 * TM_XSTR + (pt + kh) * TM_HW + kw];
#pragma unroll
                    for (int pt = 0; pt < 4; ++pt) acc[pt] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, bv[pt], acc[pt], 0, 0, 0);
                }
    }
    const int ox = tx * 16 + l16;
    if (kq != 0 || ox >= a.W) return;   // rows 0..2 of the result tile are with the lanes of kq = 0
#pragma unroll
    for (int pt = 0; pt < 4; ++pt) {
        const int oy = ty * 16 + wm * 4 + pt;
        if (oy < a.H)
#pragma unroll
            for (int co = 0; co < 3; ++co) a.out[(n * 3 + co) * plane + (size_t)oy * a.W + ox] = acc[pt][co] + a.w[8 * 81 * 8 * 4 + co];
    }
}

}  // namespace cid

static float hashf(unsigned long long i) {   // splitmix64 -> [-1, 1)
    unsigned long long z = i + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)((double)(z >> 11) / 9007199254740992.0 * 2.0 - 1.0);
}

template <class F>
static int time_ms(F launch, double* med) {
    hipEvent_t e0, e1;
    HIP_OK(hipEventCreate(&e0));
    HIP_OK(hipEventCreate(&e1));
    for (int i = 0; i < 3; ++i) launch();
    HIP_OK(hipDeviceSynchronize());
    std::vector<double> t;
    for (int r = 0; r < 5; ++r) {
        HIP_OK(hipEventRecord(e0));
        for (int i = 0; i < 10; ++i) launch();
        HIP_OK(hipEventRecord(e1));
        HIP_OK(hipEventSynchronize(e1));
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, e0, e1));
        t.push_back(ms / 10);
    }
    std::sort(t.begin(), t.end());
    *med = t[2];
    HIP_OK(hipGetLastError());
    return 0;
}

int main(int argc, char** argv) {
    using namespace cid;
    const int N = argc > 3 ? std::atoi(argv[1]) : 16, H = argc > 3 ? std::atoi(argv[2]) : 256, W = argc > 3 ? std::atoi(argv[3]) : 256;
    if (N < 1 || N > 65535 || H < 1 || W < 1 || (long long)H * W > (1 << 24)) { std::fprintf(stderr, "bad shape\n"); return 2; }
    const size_t plane = (size_t)H * W, nin = (size_t)N * 64 * plane, nout = (size_t)N * 3 * plane;
    std::vector<float> hin(nin), w(3 * 64 * 81), bias = {0.1f, -0.2f, 0.3f};
    for (size_t i = 0; i < nin; ++i) hin[i] = hashf(i);
    for (size_t i = 0; i < w.size(); ++i) w[i] = hashf((1ull << 40) + i) * 0.0139f;   // +-sqrt(1 / 5184)
    std::vector<float> wv((size_t)E_TAIL_W + 64, 0.f), wm((size_t)8 * 81 * 8 * 4 + 4, 0.f);
    for (int co = 0; co < 3; ++co)
        for (int ci = 0; ci < 64; ++ci)
            for (int kh = 0; kh < 9; ++kh)
                for (int kw = 0; kw < 9; ++kw) {
                    const float v = w[(((size_t)co * 64 + ci) * 9 + kh) * 9 + kw];
                    wv[((size_t)ci * 9 + kh) * E_TAIL_WROW + co * 9 + kw] = v;
                    wm[(((size_t)(ci / 8) * 81 + kh * 9 + kw) * 8 + ci % 8) * 4 + co] = v;
                }
    for (int co = 0; co < 3; ++co) wv[E_TAIL_W + co] = wm[(size_t)8 * 81 * 8 * 4 + co] = bias[co];
    float *din, *dwv, *dwm, *o1, *o2;
    HIP_OK(hipMalloc(&din, nin * 4));
    HIP_OK(hipMalloc(&dwv, wv.size() * 4));
    HIP_OK(hipMalloc(&dwm, wm.size() * 4));
    HIP_OK(hipMalloc(&o1, nout * 4));
    HIP_OK(hipMalloc(&o2, nout * 4));
    HIP_OK(hipMemcpy(din, hin.data(), nin * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dwv, wv.data(), wv.size() * 4, hipMemcpyHostToDevice));
    HIP_OK(hipMemcpy(dwm, wm.data(), wm.size() * 4, hipMemcpyHostToDevice));
    const int vtx = (W + E_TAIL_TW - 1) / E_TAIL_TW, vt = ((H + E_TAIL_TH - 1) / E_TAIL_TH) * vtx;
    const int mtx = (W + 15) / 16, mt = ((H + 15) / 16) * mtx;
    const EsrTailArgs va{din, o1, dwv, H, W, vtx, 0};
    const EsrTailMfmaArgs ma{din, o2, dwm, H, W, mtx, 0};
    const auto valu = [&] { hipLaunchKernelGGL(k_esr_tail<false>, dim3(vt, N), dim3(E_TAIL_THREADS), 0, 0, va); };
    const auto mfma = [&] { hipLaunchKernelGGL(k_esr_tail_mfma, dim3(mt, N), dim3(D_THREADS), 0, 0, ma); };
    double tv = 0, tm = 0;
    if (time_ms(valu, &tv)) return 1;
    if (time_ms(mfma, &tm)) return 1;
    std::vector<float> h1(nout), h2(nout);
    HIP_OK(hipMemcpy(h1.data(), o1, nout * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(h2.data(), o2, nout * 4, hipMemcpyDeviceToHost));
    double dmax = 0, amax = 0;
    for (size_t i = 0; i < nout; ++i) {
        dmax = std::max(dmax, (double)std::fabs(h1[i] - h2[i]));
        amax = std::max(amax, (double)std::fabs(h1[i]));
    }
    const double gflop = 2.0 * N * plane * 5184 * 3 / 1e9;
    std::printf("tail B=%d %dx%d %.1f GFLOP | VALU k_esr_tail %.3f ms %.1f TF/s | MFMA 16x16x4 (3 of 16 rows) %.3f ms %.1f TF/s | MFMA/VALU %.2f | "
                "max|valu - mfma| %.3e of max|out| %.3f\n", N, H, W, gflop, tv, gflop / tv, tm, gflop / tm, tm / tv, dmax, amax);
    return dmax <= 1e-4 * std::max(1.0, amax) ? 0 : 3;
}
