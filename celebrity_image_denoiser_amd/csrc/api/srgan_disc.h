// The SRGAN trainer's discriminator (cid_srd_*): weight packing, workspace plan and the forward's launches.  Layers model.0 ... model.10
// are the denoise discriminator's and run on its kernels and launch helpers (disc_forward.h); model.11 runs on k_disc_conv as two
// 128-channel halves; the rest is in srgan_disc_kernels.h.  Host code.
#pragma once
#include "disc_forward.h"
#include "../srgan_disc_kernels.h"

namespace {

constexpr int kSrdConvs = 7;
constexpr DiscConvDef kSrdConv[kSrdConvs] = {
    {"model.0", 3, 64, 3, 1},      {"model.2", 64, 64, 3, 2},    {"model.5", 64, 128, 3, 1},  {"model.8", 128, 128, 3, 2},
    {"model.11", 128, 256, 3, 1},  {"model.15", 256, 512, 1, 1}, {"model.17", 512, 1, 1, 1},
};
constexpr int kSrdBnC[SRD_BNS] = {64, 128, 128, 256};
constexpr int kSrdHalf = 128;   // channels per workgroup of model.11: k_disc_conv<128, 128, 1, ., ., 256>

// Blob segments (floats, each 64-float aligned): weights then biases of each convolution.  model.0, model.15 and model.17 keep the
// reference layout; model.2, 5, 8 are packed [CIN/8][9 taps][8][COUT] with the biases right behind; model.11 is two such blocks, one
// per half: [16][9][8][128] of output channels 128*half ... 128*half + 127, then their 128 biases.
struct SrdBlob {
    size_t off[kSrdConvs], total;
    SrdBlob() : off{}, total(0) {
        size_t at = 0;
        for (int i = 0; i < kSrdConvs; ++i) {
            off[i] = at;
            const auto& L = kSrdConv[i];
            at = align64(at + (size_t)L.cout * L.cin * L.k * L.k + L.cout);
        }
        total = at;
    }
};
const SrdBlob kSrdBlob;

struct SrdPlan {
    int H2, W2, H4, W4;
    int tiles_x[SRD_BNS], tiles[SRD_BNS];   // conv launches 2, 5, 8, 11
    size_t regA, regB, st, slab[SRD_BNS], total;
};

constexpr int kSrdTileRows[SRD_BNS] = {DiscGeom<64, 64, 2>::TH, DiscGeom<64, 128, 1>::TH, DiscGeom<128, 128, 2>::TH,
                                       DiscGeom<128, kSrdHalf, 1>::TH};

int srd_plan(int N, int H, int W, int training, SrdPlan& p) {
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;   // the layer-0 kernel indexes an image's pixels with int
    p.H2 = (H - 1) / 2 + 1;
    p.W2 = (W - 1) / 2 + 1;
    p.H4 = (p.H2 - 1) / 2 + 1;
    p.W4 = (p.W2 - 1) / 2 + 1;
    if (training && (long long)N * p.H4 * p.W4 == 1) return CID_ERR_SHAPE;
    const int ho[SRD_BNS] = {p.H2, p.H2, p.H4, p.H4}, wo[SRD_BNS] = {p.W2, p.W2, p.W4, p.W4};
    for (int l = 0; l < SRD_BNS; ++l) {
        p.tiles_x[l] = (wo[l] + D_TW - 1) / D_TW;
        p.tiles[l] = ((ho[l] + kSrdTileRows[l] - 1) / kSrdTileRows[l]) * p.tiles_x[l];
    }
    const size_t n = (size_t)N, f = sizeof(float);
    // region A: a0 (64 x H x W), later z5 (128 x H2 x W2), later z11 (256 x H4 x W4); region B: z2 (64 x H2 x W2), later z8 (128 x H4 x W4)
    const size_t a = std::max({n * 64 * H * W, n * 128 * p.H2 * p.W2, n * 256 * p.H4 * p.W4}) * f;
    const size_t b = std::max(n * 64 * p.H2 * p.W2, n * 128 * p.H4 * p.W4) * f;
    size_t at = 0;
    p.regA = take(at, a);
    p.regB = take(at, b);
    p.st = take(at, (size_t)SRD_BNS * SRD_BN_MAXC * 2 * f);
    for (int l = 0; l < SRD_BNS; ++l) {
        p.slab[l] = at;
        if (training) at += align256((size_t)kSrdBnC[l] * 2 * n * p.tiles[l] * sizeof(double));
    }
    p.total = at;
    return CID_OK;
}

}  // namespace

struct cid_srd_s : HandleBase {
    std::vector<float> staging = std::vector<float>(kSrdBlob.total, 0.f);
    bool have[kSrdConvs][2] = {};
};

namespace {
// Where one forward keeps its tensors: two overlapping workspace regions (cid_srd_forward); a saved-buffer entry point fills the
// same struct from a per-call buffer.
struct SrdBufs {
    float *a0, *z2, *z5, *z8, *z11;
    float* st[SRD_BNS];      // (scale, shift) pairs of the four BatchNorms
    double* slab[SRD_BNS];   // train mode: per-tile partial sums
    double* mi[SRD_BNS];     // (mean, invstd) pairs, or null
    double *pooled, *hidden; // the head's 256 pooled means and 512 hidden pre-activations per image, or null (both or neither)
};

// The forward's launch sequence on checked arguments.
int srd_forward_run(const Call& cx, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, int training,
                    const SrdPlan& p, const SrdBufs& b) {
    const float* blob = cx.h->dev_blob;
    const hipStream_t s = cx.s;

    if (!training) {
        SrdBnEvalArgs e{};
        for (int l = 0; l < SRD_BNS; ++l) {
            e.gamma[l] = bn[l].gamma;
            e.beta[l] = bn[l].beta;
            e.running_mean[l] = bn[l].running_mean;
            e.running_var[l] = bn[l].running_var;
            e.eps[l] = bn[l].eps;
            e.st[l] = b.st[l];
            e.C[l] = kSrdBnC[l];
        }
        if (b.mi[0]) {
            SrdBnEvalSavedArgs es{e, {b.mi[0], b.mi[1], b.mi[2], b.mi[3]}};
            hipLaunchKernelGGL(k_srd_bn_eval_saved, dim3(SRD_BNS), dim3(SRD_BN_MAXC), 0, s, es);
        } else {
            hipLaunchKernelGGL(k_srd_bn_eval, dim3(SRD_BNS), dim3(SRD_BN_MAXC), 0, s, e);
        }
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn_eval");
    }
    // layer 0
    if (const int rc = disc_conv0_launches(cx, in, in_fmt, b.a0, blob + kSrdBlob.off[0], N, H, W)) return rc;
    const auto stats = [&](int l, long long pix) {
        return disc_stats_launch(bn[l], kSrdBnC[l], b.slab[l], (long long)N * p.tiles[l], (double)N * (double)pix, b.st[l], b.mi[l], s);
    };
    const auto conv_args = [&](const float* src, float* dst, int ci, const float* st_in, int l, int Hin, int Win, int Ho, int Wo) {
        return disc_conv_args(src, dst, blob + kSrdBlob.off[ci], st_in, training ? b.slab[l] : nullptr, (long long)N * p.tiles[l], Hin,
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
    // layer 11 (reads z8 through BN9 + LeakyReLU, writes z11 in two 128-channel halves), BN12
    if (disc_conv_launch<128, kSrdHalf, 1, true, 256>(conv_args(b.z8, b.z11, 4, b.st[2], 3, p.H4, p.W4, p.H4, p.W4), 3, p, N, training, s) !=
        hipSuccess)
        return cx.hip("conv11");
    if (training && stats(3, (long long)p.H4 * p.W4) != hipSuccess) return cx.hip("bn12 stats");
    // head: BN12 + LeakyReLU, average pool, the two 1x1 convolutions, sigmoid
    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        SrdHeadArgs a{b.z11, b.st[3], blob + kSrdBlob.off[5], blob + kSrdBlob.off[6], out, (long long)p.H4 * p.W4, n0};
        if (b.pooled) {
            SrdHeadSavedArgs as{a, b.pooled, b.hidden};
            hipLaunchKernelGGL(k_srd_head_saved, dim3((unsigned)n), dim3(SRD_HEAD_THREADS), 0, s, as);
        } else {
            hipLaunchKernelGGL(k_srd_head, dim3((unsigned)n), dim3(SRD_HEAD_THREADS), 0, s, a);
        }
    })) return rc;
    if (training) {
        SrdBnCountArgs c{};
        for (int l = 0; l < SRD_BNS; ++l) c.count[l] = reinterpret_cast<long long*>(bn[l].num_batches_tracked);
        hipLaunchKernelGGL(k_srd_bn_count, dim3(1), dim3(64), 0, s, c);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn count");
    }
    return CID_OK;
}
}  // namespace

extern "C" {

int cid_srd_create(cid_srd_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = new (std::nothrow) cid_srd_s();
    return *out ? CID_OK : CID_ERR_INVALID;
}

void cid_srd_destroy(cid_srd_t d) { delete d; }

const char* cid_srd_last_error(cid_srd_t d) { return d ? d->err.c_str() : "null handle"; }

int cid_srd_set_weight(cid_srd_t d, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!d) return CID_ERR_INVALID;
    if (!key || !data || (!shape && ndim > 0)) return d->fail(CID_ERR_INVALID, "cid_srd_set_weight: null argument");
    const std::string k(key);
    int li = -1, is_bias = 0;
    for (int i = 0; i < kSrdConvs; ++i) {
        if (k == std::string(kSrdConv[i].name) + ".weight") { li = i; is_bias = 0; }
        if (k == std::string(kSrdConv[i].name) + ".bias") { li = i; is_bias = 1; }
    }
    if (li < 0)
        return d->fail(CID_ERR_KEY, "cid_srd_set_weight: unknown key '" + k +
                                        "' (BatchNorm tensors model.3/6/9/12 are passed to cid_srd_forward, not staged)");
    const auto& L = kSrdConv[li];
    const int64_t want_w[4] = {L.cout, L.cin, L.k, L.k};
    const bool ok = is_bias ? (ndim == 1 && shape[0] == L.cout)
                            : (ndim == 4 && std::equal(shape, shape + 4, want_w));
    if (!ok) return d->fail(CID_ERR_SHAPE, "cid_srd_set_weight: size mismatch for " + k);
    float* seg = d->staging.data() + kSrdBlob.off[li];
    const size_t nw = (size_t)L.cout * L.cin * L.k * L.k;
    // the MFMA layers: `part` output channels per block of [CIN/8][9][8][part] weights + part biases (one block, or model.11's two halves)
    const int part = li == 4 ? kSrdHalf : L.cout;
    const size_t block = (size_t)L.cin * 9 * part + part;
    if (L.k == 1 || li == 0) {
        std::memcpy(is_bias ? seg + nw : seg, data, (is_bias ? (size_t)L.cout : nw) * sizeof(float));
    } else if (is_bias) {
        for (int co = 0; co < L.cout; ++co) seg[(size_t)(co / part) * block + (size_t)L.cin * 9 * part + co % part] = data[co];
    } else {
        for (int co = 0; co < L.cout; ++co)
            for (int ci = 0; ci < L.cin; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    seg[(size_t)(co / part) * block + ((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * part + co % part] =
                        data[((size_t)co * L.cin + ci) * 9 + tap];
    }
    d->have[li][is_bias] = true;
    return CID_OK;
}

size_t cid_srd_packed_weights_bytes(void) { return kSrdBlob.total * sizeof(float); }

int cid_srd_upload_weights(cid_srd_t d, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    if (!device_blob) return d->fail(CID_ERR_INVALID, "cid_srd_upload_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return d->fail(CID_ERR_WORKSPACE, "cid_srd_upload_weights: blob must be 256-byte aligned");
    for (int i = 0; i < kSrdConvs; ++i)
        if (!d->have[i][0] || !d->have[i][1])
            return d->fail(CID_ERR_STATE, std::string("cid_srd_upload_weights: ") + kSrdConv[i].name + " not set");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(device_blob, d->staging.data(), kSrdBlob.total * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // staging is pageable host memory owned by the handle
    if (e != hipSuccess) return d->fail(CID_ERR_HIP, std::string("cid_srd_upload_weights: ") + hipGetErrorString(e));
    d->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_srd_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    SrdPlan p;
    return plan_bytes(srd_plan(N, H, W, training, p), p, bytes);
}

int cid_srd_forward(cid_srd_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, int training,
                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, "cid_srd_forward", stream);
    SrdPlan p;
    if (const int rc = disc_check_args(cx, in, in_fmt, out, N, H, W, bn, SRD_BNS, training, workspace,
                                       [&] { return srd_plan(N, H, W, training, p); }))
        return rc;
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_srd_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    char* ws = static_cast<char*>(workspace);
    SrdBufs b{};
    b.a0 = b.z5 = b.z11 = reinterpret_cast<float*>(ws + p.regA);
    b.z2 = b.z8 = reinterpret_cast<float*>(ws + p.regB);
    for (int l = 0; l < SRD_BNS; ++l) {
        b.st[l] = reinterpret_cast<float*>(ws + p.st) + l * SRD_BN_MAXC * 2;
        b.slab[l] = reinterpret_cast<double*>(ws + p.slab[l]);
    }
    return srd_forward_run(cx, in, in_fmt, out, N, H, W, bn, training, p, b);
}

int cid_srd_losses(const float* p_real, const float* p_fake, int N, double* out, void* stream) {
    if (!p_real || !p_fake || !out) return CID_ERR_INVALID;
    if (((uintptr_t)p_real & 3) || ((uintptr_t)p_fake & 3) || ((uintptr_t)out & 7)) return CID_ERR_INVALID;
    if (N < 1) return CID_ERR_SHAPE;
    SrdLossArgs a{p_real, p_fake, N, out};
    hipLaunchKernelGGL(k_srd_losses, dim3(1), dim3(D_LOSS_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
