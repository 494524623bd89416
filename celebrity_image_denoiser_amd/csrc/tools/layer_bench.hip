// layer_bench.hip — timing experiments on single layers of the forward (not part of the product).
// Build: make -C celebrity_image_denoiser_amd/csrc tools     Run on the GPU box: ./layer_bench
// Each variant is run ROUNDS times, interleaved with the others in one process; prints median ms
// and algorithmic TFLOP/s.
#include "../conv_kernels.h"
#include "../wino64_kernels.h"
#include "../wino42_kernels.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <functional>
#include <string>
#include <vector>

using namespace cid;
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { std::fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); std::exit(1); } } while (0)

struct Variant { std::string name; std::function<void(hipStream_t)> run; double flops; };

static float* dalloc(size_t n, float scale) {
    std::vector<float> h(n);
    uint32_t s = 12345u + (uint32_t)n;
    for (size_t i = 0; i < n; ++i) { s = s * 1664525u + 1013904223u; h[i] = scale * ((int)(s >> 8) % 2001 - 1000) / 1000.0f; }
    float* d; CK(hipMalloc(&d, n * sizeof(float)));
    CK(hipMemcpy(d, h.data(), n * sizeof(float), hipMemcpyHostToDevice));
    return d;
}

template <int CIN, int COUT, int MODE>
static Variant make(const char* name, int N, int H, int W, float* in, float* w, float* bias, float* out, float* pool) {
    GemmConvArgs a{};
    a.in = in; a.w = w; a.bias = bias; a.out = out; a.pool = pool;
    a.N = N; a.Hin = H; a.Win = W; a.in_ps = CIN; a.Hc = H; a.Wc = W; a.Hs = H; a.Ws = W; a.out_ps = COUT; a.out_coff = 0;
    a.tiles_x = (W + TILE_W - 1) / TILE_W; a.tiles_y = (H + TILE_H - 1) / TILE_H;
    a.tiles_total = N * a.tiles_x * a.tiles_y; a.tiles_per_xcd = (a.tiles_total + 7) / 8;
    a.rcp_x = tile_rcp(a.tiles_x); a.rcp_xy = tile_rcp(a.tiles_x * a.tiles_y);
    constexpr int NB = (MODE == 2 ? 4 * COUT : COUT) / NTILE;
    const int grid = 8 * a.tiles_per_xcd * NB;
    const double flops = 2.0 * CIN * COUT * (MODE == 2 ? 4 : 9) * (double)N * H * W;
    return {name, [=](hipStream_t s) { hipLaunchKernelGGL((k_gemm_conv<CIN, COUT, MODE>), dim3(grid), dim3(THREADS), 0, s, a); }, flops};
}

template <int CIN, int COUT, bool POOL, int TC>
static Variant makew64(const char* name, int N, int H, int W, float* in, float* u, float* bias, float* out, float* pool) {
    WinoArgs a{};
    a.in = in; a.u = u; a.bias = bias; a.out = out; a.pool = pool;
    static unsigned* tabs[2] = {nullptr, nullptr};
    const int ti = TC == 32 ? 0 : 1;
    if (!tabs[ti]) {
        std::vector<unsigned> h(wino_slot_table(TC, 32 / TC, nullptr));
        wino_slot_table(TC, 32 / TC, h.data());
        CK(hipMalloc(&tabs[ti], h.size() * 4));
        CK(hipMemcpy(tabs[ti], h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    a.slot_tab = tabs[ti];
    a.N = N; a.Hin = H; a.Win = W; a.in_ps = CIN; a.Hc = H; a.Wc = W; a.Hs = H; a.Ws = W; a.out_ps = COUT; a.out_coff = 0;
    constexpr int TRW = 32 / TC;
    a.tiles_x = (W + 2 * TC - 1) / (2 * TC); a.tiles_y = (H + 2 * TRW - 1) / (2 * TRW);
    a.tiles_total = N * a.tiles_x * a.tiles_y; a.tiles_per_xcd = (a.tiles_total + 7) / 8;
    a.rcp_x = tile_rcp(a.tiles_x); a.rcp_xy = tile_rcp(a.tiles_x * a.tiles_y);
    const int grid = 8 * a.tiles_per_xcd * (COUT / WN2);
    const double flops = 2.0 * CIN * COUT * 9 * (double)N * H * W;   // algorithmic (direct) FLOPs
    return {name, [=](hipStream_t s) { hipLaunchKernelGGL((k_wino64_conv<CIN, COUT, POOL, TC>), dim3(grid), dim3(THREADS), 0, s, a); }, flops};
}

template <int CIN, int COUT, bool POOL, int TC>
static Variant makew42(const char* name, int N, int H, int W, float* in, float* u, float* bias, float* out, float* pool) {
    WinoArgs a{};
    a.in = in; a.u = u; a.bias = bias; a.out = out; a.pool = pool;
    std::vector<unsigned> h(wino42_slot_table<TC>(nullptr));
    wino42_slot_table<TC>(h.data());
    unsigned* tab; CK(hipMalloc(&tab, h.size() * 4));
    CK(hipMemcpy(tab, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    a.slot_tab = tab;
    a.N = N; a.Hin = H; a.Win = W; a.in_ps = CIN; a.Hc = H; a.Wc = W; a.Hs = H; a.Ws = W; a.out_ps = COUT; a.out_coff = 0;
    constexpr int TRW = 16 / TC;
    a.tiles_x = (W + 4 * TC - 1) / (4 * TC); a.tiles_y = (H + 2 * TRW - 1) / (2 * TRW);
    a.tiles_total = N * a.tiles_x * a.tiles_y; a.tiles_per_xcd = (a.tiles_total + 7) / 8;
    a.rcp_x = tile_rcp(a.tiles_x); a.rcp_xy = tile_rcp(a.tiles_x * a.tiles_y);
    const int grid = 8 * a.tiles_per_xcd * (COUT / WN2);
    const double flops = 2.0 * CIN * COUT * 9 * (double)N * H * W;   // algorithmic (direct) FLOPs
    return {name, [=](hipStream_t s) { hipLaunchKernelGGL((k_wino42_conv<CIN, COUT, POOL, TC>), dim3(grid), dim3(THREADS), 0, s, a); }, flops};
}

int main(int argc, char** argv) {
    const int N = argc > 1 ? std::atoi(argv[1]) : 256;
    const int ROUNDS = 7;
    hipStream_t s; CK(hipStreamCreate(&s));
    // upconv1.0 shape: 128 -> 64 @ 128x128 ; bottleneck.2 shape: 256 -> 256 @ 32x32
    float* inA = dalloc((size_t)N * 128 * 128 * 128, 1.f);
    float* wA = dalloc((size_t)128 * 64 * 9, 0.05f);
    float* bA = dalloc(64, 0.1f);
    float* outA = dalloc((size_t)N * 128 * 128 * 64, 0.f);
    float* poolA = dalloc((size_t)N * 64 * 64 * 64, 0.f);
    float* inB = dalloc((size_t)N * 32 * 32 * 256, 1.f);
    float* wB = dalloc((size_t)256 * 256 * 9, 0.05f);
    float* bB = dalloc(256, 0.1f);
    float* outB = dalloc((size_t)N * 32 * 32 * 256, 0.f);
    std::vector<Variant> v;
    float* uA = dalloc((size_t)128 * 64 * 16, 0.05f);
    float* uB = dalloc((size_t)256 * 256 * 16, 0.05f);
    float* u42A = dalloc((size_t)128 * 64 * 24, 0.05f);
    float* u42B = dalloc((size_t)256 * 256 * 24, 0.05f);
    v.push_back(make<128, 64, 0>("A direct 128->64@128", N, 128, 128, inA, wA, bA, outA, poolA));
    v.push_back(makew64<128, 64, false, 32>("A wino64 base", N, 128, 128, inA, uA, bA, outA, poolA));
    v.push_back(makew42<128, 64, false, 8>("A wino42 base", N, 128, 128, inA, u42A, bA, outA, poolA));
    v.push_back(makew42<256, 256, false, 8>("B wino42 base", N, 32, 32, inB, u42B, bB, outB, nullptr));
    v.push_back(make<256, 256, 0>("B direct 256->256@32", N, 32, 32, inB, wB, bB, outB, nullptr));
    v.push_back(makew64<256, 256, false, 16>("B wino64 base", N, 32, 32, inB, uB, bB, outB, nullptr));
    // up1 shape: ConvT 128 -> 64 on 64x64 inputs (output 128x128x64); reuse inA (>= N*64*64*128) and outA
    v.push_back(make<128, 64, 2>("T convT 128->64@64 base", N, 64, 64, inA, wA, bA, outA, nullptr));
    std::vector<std::vector<float>> ms(v.size());
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (auto& x : v) x.run(s);   // warm-up
    CK(hipStreamSynchronize(s));
    for (int r = 0; r < ROUNDS; ++r)
        for (size_t i = 0; i < v.size(); ++i) {
            CK(hipEventRecord(e0, s)); v[i].run(s); CK(hipEventRecord(e1, s)); CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1)); ms[i].push_back(t);
        }
    CK(hipGetLastError());
    for (size_t i = 0; i < v.size(); ++i) {
        std::sort(ms[i].begin(), ms[i].end());
        const float med = ms[i][ms[i].size() / 2];
        std::printf("%-28s median %8.4f ms  min %8.4f ms  %7.2f TFLOP/s  (%.1f%% of 157.3 algorithmic)\n", v[i].name.c_str(), med, ms[i][0],
                    v[i].flops / (med * 1e-3) / 1e12, 100.0 * v[i].flops / (med * 1e-3) / 1e12 / 157.3);
    }
    return 0;
}
