// The trainer's discriminator (cid_disc_*): weight packing, workspace plan and the forward's launches; kernels in disc_kernels.h.  Host code.
#pragma once
#include "../api_common.h"
#include "../disc_kernels.h"

namespace {

struct DiscConvDef { const char* name; int cin, cout, k, stride; };
constexpr int kDiscConvs = 5;
constexpr DiscConvDef kDiscConv[kDiscConvs] = {
    {"model.0", 3, 64, 3, 1}, {"model.2", 64, 64, 3, 2}, {"model.5", 64, 128, 3, 1}, {"model.8", 128, 128, 3, 2}, {"model.12", 128, 1, 1, 1},
};
constexpr int kDiscBnC[3] = {64, 128, 128};

// Blob segments (floats, each 64-float aligned): weights then biases of each convolution.  Layer 0 and 12 keep the reference
// layout; layers 2, 5, 8 are packed [CIN/8][9 taps][8][COUT] (DiscConvArgs::w) with the biases right behind.
struct DiscBlob {
    size_t off[kDiscConvs], total;
    DiscBlob() : off{}, total(0) {
        size_t at = 0;
        for (int i = 0; i < kDiscConvs; ++i) {
            off[i] = at;
            const auto& L = kDiscConv[i];
            at += (size_t)L.cout * L.cin * L.k * L.k + L.cout;
            at = (at + 63) & ~(size_t)63;
        }
        total = at;
    }
};
const DiscBlob kDiscBlob;

struct DiscPlan {
    int H2, W2, H4, W4;
    int tiles_x[3], tiles[3];           // conv launches 2, 5, 8
    size_t regA, regB, st, slab[3], total;
};

constexpr int kDiscTileRows[3] = {DiscGeom<64, 64, 2>::TH, DiscGeom<64, 128, 1>::TH, DiscGeom<128, 128, 2>::TH};

int disc_plan(int N, int H, int W, int training, DiscPlan& p) {
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;   // the layer-0 kernel indexes an image's pixels with int
    p.H2 = (H - 1) / 2 + 1;
    p.W2 = (W - 1) / 2 + 1;
    p.H4 = (p.H2 - 1) / 2 + 1;
    p.W4 = (p.W2 - 1) / 2 + 1;
    if (training && (long long)N * p.H4 * p.W4 == 1) return CID_ERR_SHAPE;
    const int ho[3] = {p.H2, p.H2, p.H4}, wo[3] = {p.W2, p.W2, p.W4};
    for (int l = 0; l < 3; ++l) {
        p.tiles_x[l] = (wo[l] + D_TW - 1) / D_TW;
        p.tiles[l] = ((ho[l] + kDiscTileRows[l] - 1) / kDiscTileRows[l]) * p.tiles_x[l];
    }
    const size_t n = (size_t)N, f = sizeof(float);
    // region A: a0 (64 x H x W), later z5 (128 x H2 x W2); region B: z2 (64 x H2 x W2), later z8 (128 x H4 x W4)
    const size_t a = std::max(n * 64 * H * W, n * 128 * p.H2 * p.W2) * f;
    const size_t b = std::max(n * 64 * p.H2 * p.W2, n * 128 * p.H4 * p.W4) * f;
    size_t at = 0;
    p.regA = take(at, a);
    p.regB = take(at, b);
    p.st = take(at, 3 * 128 * 2 * f);
    const int couts[3] = {64, 128, 128};
    for (int l = 0; l < 3; ++l) {
        p.slab[l] = at;
        if (training) at += align256((size_t)couts[l] * 2 * n * p.tiles[l] * sizeof(double));
    }
    p.total = at;
    return CID_OK;
}

// One MFMA convolution layer over a plan's tiles (DiscPlan, or the SRGAN discriminator's plan).  COUT_TOTAL > COUT: the layer's
// COUT-channel parts are the grid's z (k_disc_conv).
template <int CIN, int COUT, int S, bool BN_IN, int COUT_TOTAL = COUT, class Plan>
hipError_t disc_conv_launch(const DiscConvArgs& base, int layer, const Plan& p, int N, bool training, hipStream_t s) {
    (void)for_each_launch(N, [&](int n0, int n) {
        DiscConvArgs a = base;
        a.n0 = n0;
        a.tiles_x = p.tiles_x[layer];
        a.tiles = p.tiles[layer];
        const dim3 grid((unsigned)p.tiles[layer], (unsigned)n, COUT_TOTAL / COUT), block(D_THREADS);
        if (training) hipLaunchKernelGGL((k_disc_conv<CIN, COUT, S, BN_IN, true, COUT_TOTAL>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_disc_conv<CIN, COUT, S, BN_IN, false, COUT_TOTAL>), grid, block, 0, s, a);
    });
    return hipGetLastError();
}

bool disc_finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

// The tensors of one MFMA convolution launch: `w` its packed weights, `slab` null in eval mode, `rows` = N * tiles of the layer.
DiscConvArgs disc_conv_args(const float* src, float* dst, const float* w, const float* st_in, double* slab, long long rows, int Hin,
                            int Win, int Ho, int Wo) {
    DiscConvArgs a{};
    a.in = src;
    a.out = dst;
    a.w = w;
    a.st_in = st_in;
    a.slab = slab;
    a.rows = rows;
    a.Hin = Hin;
    a.Win = Win;
    a.Ho = Ho;
    a.Wo = Wo;
    return a;
}

// Train-mode statistics of one C-channel BatchNorm from its layer's slab: (scale, shift) into `st`, the running buffers updated.
hipError_t disc_stats_launch(const cid_disc_bn& bn, int C, const double* slab, long long rows, double count, float* st, double* mi,
                             hipStream_t s) {
    DiscStatsArgs a{};
    a.slab = slab;
    a.rows = rows;
    a.count = count;
    a.gamma = bn.gamma;
    a.beta = bn.beta;
    a.running_mean = bn.running_mean;
    a.running_var = bn.running_var;
    a.num_batches_tracked = reinterpret_cast<const long long*>(bn.num_batches_tracked);
    a.eps = bn.eps;
    a.momentum = bn.momentum == CID_DISC_MOMENTUM_NONE ? -1.0 : bn.momentum;
    a.st = st;
    a.mi = mi;
    hipLaunchKernelGGL(k_disc_bn_stats, dim3(C), dim3(D_THREADS), 0, s, a);
    return hipPeekAtLastError();
}

// The layer-0 launches (model.0 + LeakyReLU -> a0), shared with the SRGAN discriminator.
int disc_conv0_launches(const Call& cx, const void* in, int in_fmt, float* a0, const float* w, int N, int H, int W) {
    return cx.launches(N, "conv0", [&](int n0, int n) {
        DiscConv0Args a{in, a0, w, H, W, n0};
        const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), (unsigned)n);
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_disc_conv0<true>, grid, dim3(D_THREADS), 0, cx.s, a);
        else hipLaunchKernelGGL(k_disc_conv0<false>, grid, dim3(D_THREADS), 0, cx.s, a);
    });
}

}  // namespace

struct cid_disc_s : HandleBase {
    std::vector<float> staging = std::vector<float>(kDiscBlob.total, 0.f);
    bool have[kDiscConvs][2] = {};
};

namespace {
// Where one forward keeps its tensors: two overlapping workspace regions (cid_disc_forward) or a per-call buffer (cid_disc_forward_saved).
struct DiscBufs {
    float *a0, *z2, *z5, *z8;
    float* st[3];      // (scale, shift) pairs of the three BatchNorms
    double* mi[3];     // (mean, invstd) pairs, or null
    double* slab[3];   // train mode: per-tile partial sums
};

// The argument checks every forward entry point of the two discriminators shares, in the order cid.h documents; `buf` is its
// workspace or saved buffer, bn[0 .. nbn-1] its BatchNorms and plan() its family's plan function on (N, H, W, training).
template <class PlanFn>
int disc_check_args(const Call& cx, const void* in, int in_fmt, const float* out, int N, int H, int W, const cid_disc_bn* bn, int nbn,
                    int training, const void* buf, PlanFn&& plan) {
    if (!in || !out || !bn || !buf) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) return cx.fail(CID_ERR_INVALID, "unknown input format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || ((uintptr_t)out & 3))
        return cx.fail(CID_ERR_INVALID, "misaligned fp32 operand");
    if (training != 0 && training != 1) return cx.fail(CID_ERR_INVALID, "training must be 0 or 1");
    for (int l = 0; l < nbn; ++l) {
        const cid_disc_bn& b = bn[l];
        if (!b.gamma || !b.beta || !b.running_mean || !b.running_var || (training && !b.num_batches_tracked))
            return cx.fail(CID_ERR_INVALID, "null BatchNorm pointer");
        if (!disc_finite_nonneg(b.eps)) return cx.fail(CID_ERR_INVALID, "eps must be finite and >= 0");
        if (training && !(disc_finite_nonneg(b.momentum) || b.momentum == CID_DISC_MOMENTUM_NONE))
            return cx.fail(CID_ERR_INVALID, "momentum must be finite and >= 0, or CID_DISC_MOMENTUM_NONE");
    }
    if (plan() != CID_OK)
        return training && N >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL
                   ? cx.h->fail(CID_ERR_SHAPE, "Expected more than 1 value per channel when training")
                   : cx.fail(CID_ERR_SHAPE, "input shape not accepted (N, H, W >= 1, H*W < 2^31)");
    return CID_OK;
}

int disc_check_forward(const Call& cx, const void* in, int in_fmt, const float* out, int N, int H, int W, const cid_disc_bn* bn,
                       int training, const void* buf, DiscPlan& p) {
    return disc_check_args(cx, in, in_fmt, out, N, H, W, bn, 3, training, buf, [&] { return disc_plan(N, H, W, training, p); });
}

// The forward's launch sequence on checked arguments.
int disc_forward_run(const Call& cx, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, int training,
                     const DiscPlan& p, const DiscBufs& b) {
    const float* blob = cx.h->dev_blob;
    const hipStream_t s = cx.s;

    if (!training) {
        DiscBnEvalArgs e{};
        for (int l = 0; l < 3; ++l) {
            e.gamma[l] = bn[l].gamma;
            e.beta[l] = bn[l].beta;
            e.running_mean[l] = bn[l].running_mean;
            e.running_var[l] = bn[l].running_var;
            e.eps[l] = bn[l].eps;
            e.st[l] = b.st[l];
            e.C[l] = kDiscBnC[l];
            e.mi[l] = b.mi[l];
        }
        hipLaunchKernelGGL(k_disc_bn_eval, dim3(3), dim3(128), 0, s, e);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn_eval");
    }
    // layer 0
    if (const int rc = disc_conv0_launches(cx, in, in_fmt, b.a0, blob + kDiscBlob.off[0], N, H, W)) return rc;
    const auto stats = [&](int l, long long pix) {
        return disc_stats_launch(bn[l], kDiscBnC[l], b.slab[l], (long long)N * p.tiles[l], (double)N * (double)pix, b.st[l], b.mi[l], s);
    };
    const auto conv_args = [&](const float* src, float* dst, int ci, const float* st_in, int l, int Hin, int Win, int Ho, int Wo) {
        return disc_conv_args(src, dst, blob + kDiscBlob.off[ci], st_in, training ? b.slab[l] : nullptr, (long long)N * p.tiles[l], Hin,
                              Win, Ho, Wo);
    };
    // layer 2 (reads a0, writes z2), BN3
    if (disc_conv_launch<64, 64, 2, false>(conv_args(b.a0, b.z2, 1, nullptr, 0, H, W, p.H2, p.W2), 0, p, N, training, s) != hipSuccess)
        return cx.hip("conv2");
    if (training && stats(0, (long long)p.H2 * p.W2) != hipSuccess) return cx.hip("bn3 stats");
    // layer 5 (reads z2 through BN3 + LeakyReLU, writes z5), BN6
    if (disc_conv_launch<64, 128, 1, true>(conv_args(b.z2, b.z5, 2, b.st[0], 1, p.H2, p.W2, p.H2, p.W2), 1, p, N, training, s) != hipSuccess)
        return cx.hip("conv5");
    if (training && stats(1, (long long)p.H2 * p.W2) != hipSuccess) return cx.hip("bn6 stats");
    // layer 8 (reads z5 through BN6 + LeakyReLU, writes z8), BN9
    if (disc_conv_launch<128, 128, 2, true>(conv_args(b.z5, b.z8, 3, b.st[1], 2, p.H2, p.W2, p.H4, p.W4), 2, p, N, training, s) != hipSuccess)
        return cx.hip("conv8");
    if (training && stats(2, (long long)p.H4 * p.W4) != hipSuccess) return cx.hip("bn9 stats");
    // head: BN9 + LeakyReLU, average pool, 1x1 conv, sigmoid
    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        DiscHeadArgs a{b.z8, b.st[2], blob + kDiscBlob.off[4], out, (long long)p.H4 * p.W4, n0};
        hipLaunchKernelGGL(k_disc_head, dim3((unsigned)n), dim3(D_HEAD_THREADS), 0, s, a);
    })) return rc;
    if (training) {
        hipLaunchKernelGGL(k_disc_bn_count, dim3(1), dim3(64), 0, s, reinterpret_cast<long long*>(bn[0].num_batches_tracked),
                           reinterpret_cast<long long*>(bn[1].num_batches_tracked), reinterpret_cast<long long*>(bn[2].num_batches_tracked));
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn count");
    }
    return CID_OK;
}
}  // namespace

extern "C" {

int cid_disc_create(cid_disc_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = new (std::nothrow) cid_disc_s();
    return *out ? CID_OK : CID_ERR_INVALID;
}

void cid_disc_destroy(cid_disc_t d) { delete d; }

const char* cid_disc_last_error(cid_disc_t d) { return d ? d->err.c_str() : "null handle"; }

int cid_disc_set_weight(cid_disc_t d, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!d) return CID_ERR_INVALID;
    if (!key || !data || (!shape && ndim > 0)) return d->fail(CID_ERR_INVALID, "cid_disc_set_weight: null argument");
    const std::string k(key);
    int li = -1, is_bias = 0;
    for (int i = 0; i < kDiscConvs; ++i) {
        if (k == std::string(kDiscConv[i].name) + ".weight") { li = i; is_bias = 0; }
        if (k == std::string(kDiscConv[i].name) + ".bias") { li = i; is_bias = 1; }
    }
    if (li < 0)
        return d->fail(CID_ERR_KEY, "cid_disc_set_weight: unknown key '" + k +
                                         "' (BatchNorm tensors model.3/6/9 are passed to cid_disc_forward, not staged)");
    const auto& L = kDiscConv[li];
    const int64_t want_w[4] = {L.cout, L.cin, L.k, L.k};
    const bool ok = is_bias ? (ndim == 1 && shape[0] == L.cout)
                            : (ndim == 4 && std::equal(shape, shape + 4, want_w));
    if (!ok) return d->fail(CID_ERR_SHAPE, "cid_disc_set_weight: size mismatch for " + k);
    float* seg = d->staging.data() + kDiscBlob.off[li];
    const size_t nw = (size_t)L.cout * L.cin * L.k * L.k;
    const bool packed = li >= 1 && li <= 3;
    if (is_bias) {
        std::memcpy(seg + nw, data, (size_t)L.cout * sizeof(float));
    } else if (!packed) {
        std::memcpy(seg, data, nw * sizeof(float));
    } else {
        for (int co = 0; co < L.cout; ++co)
            for (int ci = 0; ci < L.cin; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    seg[((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * L.cout + co] = data[((size_t)co * L.cin + ci) * 9 + tap];
    }
    d->have[li][is_bias] = true;
    return CID_OK;
}

size_t cid_disc_packed_weights_bytes(void) { return kDiscBlob.total * sizeof(float); }

int cid_disc_upload_weights(cid_disc_t d, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    if (!device_blob) return d->fail(CID_ERR_INVALID, "cid_disc_upload_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return d->fail(CID_ERR_WORKSPACE, "cid_disc_upload_weights: blob must be 256-byte aligned");
    for (int i = 0; i < kDiscConvs; ++i)
        if (!d->have[i][0] || !d->have[i][1])
            return d->fail(CID_ERR_STATE, std::string("cid_disc_upload_weights: ") + kDiscConv[i].name + " not set");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(device_blob, d->staging.data(), kDiscBlob.total * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // staging is pageable host memory owned by the handle
    if (e != hipSuccess) return d->fail(CID_ERR_HIP, std::string("cid_disc_upload_weights: ") + hipGetErrorString(e));
    d->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_disc_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    return plan_bytes(disc_plan(N, H, W, training, p), p, bytes);
}

int cid_disc_forward(cid_disc_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn,
                     int training, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, "cid_disc_forward", stream);
    DiscPlan p;
    if (const int rc = disc_check_forward(cx, in, in_fmt, out, N, H, W, bn, training, workspace, p)) return rc;
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_disc_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    char* ws = static_cast<char*>(workspace);
    DiscBufs b{};
    b.a0 = b.z5 = reinterpret_cast<float*>(ws + p.regA);
    b.z2 = b.z8 = reinterpret_cast<float*>(ws + p.regB);
    for (int l = 0; l < 3; ++l) {
        b.st[l] = reinterpret_cast<float*>(ws + p.st) + l * 256;
        b.slab[l] = reinterpret_cast<double*>(ws + p.slab[l]);
    }
    return disc_forward_run(cx, in, in_fmt, out, N, H, W, bn, training, p, b);
}

}  // extern "C"
