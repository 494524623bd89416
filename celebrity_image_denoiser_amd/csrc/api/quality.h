// Image-quality metrics (cid_quality): workspace plan and launch sequence; kernels in quality_kernels.h.  Host code.
#pragma once
#include "../api_common.h"
#include "../quality_kernels.h"

namespace {

constexpr int kQualityMetrics = CID_METRIC_PSNR | CID_METRIC_SSIM | CID_METRIC_MS_SSIM;

struct QualityPlan {
    int levels;                                  // 1, or 5 with MS-SSIM
    int H[Q_LEVELS], W[Q_LEVELS], tiles_x[Q_LEVELS], tiles[Q_LEVELS], off[Q_LEVELS];
    long long slab_stride;                       // slab rows per image
    size_t pyr_a[Q_LEVELS], pyr_b[Q_LEVELS];     // byte offsets of the pooled planes of levels 1..4
    size_t total;
};

// Argument checks shared by cid_quality_workspace_bytes and cid_quality (metrics bits, then shape).
int quality_plan(int N, int H, int W, int metrics, QualityPlan& q) {
    if (metrics == 0 || (metrics & ~kQualityMetrics)) return CID_ERR_INVALID;
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((metrics & CID_METRIC_SSIM) && (H < 7 || W < 7)) return CID_ERR_SHAPE;
    if ((metrics & CID_METRIC_MS_SSIM) && (H <= 160 || W <= 160)) return CID_ERR_SHAPE;   // pytorch_msssim: min side > (11-1)*2^4
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;                            // one plane < 2^31 pixels
    q.levels = (metrics & CID_METRIC_MS_SSIM) ? Q_LEVELS : 1;
    long long rows = 0;
    int h = H, w = W;
    for (int l = 0; l < q.levels; ++l) {
        q.H[l] = h;
        q.W[l] = w;
        q.tiles_x[l] = (w + Q_TX - 1) / Q_TX;
        q.tiles[l] = ((h + Q_TY - 1) / Q_TY) * q.tiles_x[l];
        q.off[l] = (int)rows;
        rows += q.tiles[l];
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    q.slab_stride = rows;
    size_t at = align256((size_t)N * rows * QSLOTS * sizeof(double));
    for (int side = 0; side < 2; ++side)
        for (int l = 1; l < q.levels; ++l) {
            (side ? q.pyr_b : q.pyr_a)[l] = at;
            at += align256((size_t)N * 3 * q.H[l] * q.W[l] * sizeof(float));
        }
    q.total = at;
    return CID_OK;
}

// pytorch_msssim _fspecial_gauss_1d(11, 1.5) in float32: exp(-(k-5)^2 / (2*1.5^2)), normalised by its sum.
void gauss_window(float* g) {
    float sum = 0.f;
    for (int k = 0; k < 11; ++k) {
        const float d = (float)(k - 5);
        g[k] = std::exp(-(d * d) / 4.5f);
        sum += g[k];
    }
    for (int k = 0; k < 11; ++k) g[k] /= sum;
}

}  // namespace

extern "C" {

int cid_quality_workspace_bytes(int N, int H, int W, int metrics, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    QualityPlan q;
    return plan_bytes(quality_plan(N, H, W, metrics, q), q, bytes);
}

int cid_quality(const void* a, int a_fmt, const void* b, int b_fmt, int N, int H, int W, int metrics, double* out,
                void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !out || !workspace) return CID_ERR_INVALID;
    if (!fmt_ok(a, a_fmt) || !fmt_ok(b, b_fmt) || ((uintptr_t)out & 7)) return CID_ERR_INVALID;
    QualityPlan q;
    const int rc = quality_plan(N, H, W, metrics, q);
    if (rc != CID_OK) return rc;
    if (workspace_bytes < q.total || ((uintptr_t)workspace & 255)) return CID_ERR_WORKSPACE;

    static float g[11];
    static const bool g_ready = (gauss_window(g), true);
    (void)g_ready;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* part = reinterpret_cast<double*>(ws);
    const bool box = metrics & CID_METRIC_SSIM, gauss = metrics & CID_METRIC_MS_SSIM;

    (void)for_each_launch(N, [&](int n0, int nc) {   // the levels' tile launches, each checked, then the finish
        for (int l = 0; l < q.levels; ++l) {
            QualityLevelArgs p{};
            p.a = l == 0 ? a : ws + q.pyr_a[l];
            p.b = l == 0 ? b : ws + q.pyr_b[l];
            p.fa = l == 0 ? a_fmt : CID_FMT_F32_NCHW;
            p.fb = l == 0 ? b_fmt : CID_FMT_F32_NCHW;
            p.H = q.H[l];
            p.W = q.W[l];
            p.tiles_x = q.tiles_x[l];
            p.n0 = n0;
            const bool pool = gauss && l + 1 < q.levels;
            p.pa = pool ? reinterpret_cast<float*>(ws + q.pyr_a[l + 1]) : nullptr;
            p.pb = pool ? reinterpret_cast<float*>(ws + q.pyr_b[l + 1]) : nullptr;
            p.part = part + (size_t)q.off[l] * QSLOTS;
            p.slab_stride = q.slab_stride;
            std::memcpy(p.g, g, sizeof g);
            const dim3 grid((unsigned)q.tiles[l], (unsigned)nc), block(Q_THREADS);
            if (l > 0) {
                if (pool) hipLaunchKernelGGL((k_quality_tile<false, false, true, true>), grid, block, 0, s, p);
                else hipLaunchKernelGGL((k_quality_tile<false, false, true, false>), grid, block, 0, s, p);
            } else if (box && gauss) {
                hipLaunchKernelGGL((k_quality_tile<true, true, true, true>), grid, block, 0, s, p);
            } else if (gauss) {
                hipLaunchKernelGGL((k_quality_tile<true, false, true, true>), grid, block, 0, s, p);
            } else if (box) {
                hipLaunchKernelGGL((k_quality_tile<true, true, false, false>), grid, block, 0, s, p);
            } else {
                hipLaunchKernelGGL((k_quality_tile<true, false, false, false>), grid, block, 0, s, p);
            }
            if (hipPeekAtLastError() != hipSuccess) return;
        }
        QualityFinishArgs f{};
        f.part = part;
        f.slab_stride = q.slab_stride;
        f.H = H;
        f.W = W;
        for (int l = 0; l < q.levels; ++l) {
            f.level_tiles[l] = q.tiles[l];
            f.level_off[l] = q.off[l];
        }
        f.levels = q.levels;
        f.metrics = metrics;
        f.n0 = n0;
        f.out = out;
        hipLaunchKernelGGL(k_quality_finish, dim3((unsigned)nc), dim3(64), 0, s, f);
    });
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
