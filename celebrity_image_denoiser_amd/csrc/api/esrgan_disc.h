// The ESRGAN trainer's discriminator (cid_esd_*): weight packing, workspace plan, the forward's launches and the trainer's losses;
// kernels in esrgan_disc_kernels.h.  The entry points that run the forward (cid_esd_forward, cid_esd_forward_saved) are in
// esrgan_disc_backward.h, next to the backward pass.  Host code.
#pragma once
#include "../api_common.h"
#include "../esrgan_disc_kernels.h"

namespace {

struct EsdConvDef { const char* name; int cin, cout; };
constexpr int kEsdConvs = 4;
constexpr EsdConvDef kEsdConv[kEsdConvs] = {{"conv1", 3, 64}, {"conv2", 64, 128}, {"conv3", 128, 256}, {"conv4", 256, 512}};
constexpr int kEsdPt[kEsdConvs] = {0, 4, 2, 1};   // rows per wave of k_esd_conv for conv2, conv3, conv4 (tiles of 16, 8, 4 rows)
constexpr int kEsdFc = kEsdConvs;                 // index of the linear layer among the handle's five layers

inline int esd_half(int v) { return (v - 1) / 2 + 1; }
bool esd_side_ok(int H, int W) { return H >= 1 && W >= 1 && H <= CID_ESD_MAX_SIDE && W <= CID_ESD_MAX_SIDE; }

// Layer sizes of an H x W input: ho[l], wo[l] = output of conv(l + 1).
struct EsdDims {
    int ho[kEsdConvs], wo[kEsdConvs];
    EsdDims(int H, int W) {
        for (int l = 0; l < kEsdConvs; ++l) {
            ho[l] = esd_half(l ? ho[l - 1] : H);
            wo[l] = esd_half(l ? wo[l - 1] : W);
        }
    }
    size_t features() const { return (size_t)512 * ho[3] * wo[3]; }
};

// Blob segments (floats, each 64-float aligned).  conv1 keeps the reference layout, weights then biases.  conv2, conv3, conv4 are
// COUT / 64 blocks, one per 64-channel part: [CIN/8][9 taps][8][64] of output channels 64*part ... 64*part + 63, then their 64 biases.
// fc.weight is permuted into C8 order, [64 channel blocks][H4*W4][8]; fc.bias has a segment of its own.
struct EsdBlob {
    size_t off[kEsdConvs], fcw, fcb, total;
    EsdBlob(int H, int W) : off{}, fcw(0), fcb(0), total(0) {
        size_t at = 0;
        for (int i = 0; i < kEsdConvs; ++i) {
            off[i] = at;
            at = align64(at + (size_t)kEsdConv[i].cout * kEsdConv[i].cin * 9 + kEsdConv[i].cout);
        }
        fcw = at;
        at = align64(at + EsdDims(H, W).features());
        fcb = at;
        at = align64(at + 1);
        total = at;
    }
};

struct EsdPlan {
    EsdDims d;
    int tiles_x[kEsdConvs], tiles[kEsdConvs];   // conv2, conv3, conv4 (index 0 unused)
    size_t a[kEsdConvs], total;                 // a1 ... a4: four distinct regions
    EsdPlan(int H, int W) : d(H, W), tiles_x{}, tiles{}, a{}, total(0) {}
};

int esd_plan(int N, int H, int W, EsdPlan& p) {
    if (N < 1 || !esd_side_ok(H, W)) return CID_ERR_SHAPE;
    for (int l = 1; l < kEsdConvs; ++l) {
        p.tiles_x[l] = cdiv(p.d.wo[l], D_TW);
        p.tiles[l] = cdiv(p.d.ho[l], 4 * kEsdPt[l]) * p.tiles_x[l];
    }
    size_t at = 0;
    for (int l = 0; l < kEsdConvs; ++l) p.a[l] = take(at, (size_t)N * kEsdConv[l].cout * p.d.ho[l] * p.d.wo[l] * sizeof(float));
    p.total = at;
    return CID_OK;
}

}  // namespace

struct cid_esd_s : HandleBase {
    int H, W;
    EsdBlob blob;
    std::vector<float> staging;
    bool have[kEsdConvs + 1][2] = {};
    cid_esd_s(int h, int w) : H(h), W(w), blob(h, w), staging(blob.total, 0.f) {}
};

namespace {

template <int CIN, int COUT, int PT>
int esd_conv_launches(const Call& cx, const char* what, const float* src, float* dst, const float* w, int layer, const EsdPlan& p, int Hin,
                      int Win, int N) {
    return cx.launches(N, what, [&](int n0, int n) {
        const EsdConvArgs a{src, dst, w, Hin, Win, p.d.ho[layer], p.d.wo[layer], p.tiles_x[layer], n0};
        const dim3 grid((unsigned)p.tiles[layer], (unsigned)n, COUT / ESD_PART);
        hipLaunchKernelGGL((k_esd_conv<CIN, COUT, PT>), grid, dim3(D_THREADS), 0, cx.s, a);
    });
}

// The forward's launch sequence on checked arguments.
int esd_forward_run(const Call& cx, const cid_esd_s& h, const void* in, int in_fmt, float* out, int N, const EsdPlan& p, char* ws) {
    const float* blob = h.dev_blob;
    float* a[kEsdConvs];
    for (int l = 0; l < kEsdConvs; ++l) a[l] = reinterpret_cast<float*>(ws + p.a[l]);
    const EsdDims& d = p.d;
    if (const int rc = cx.launches(N, "conv1", [&](int n0, int n) {
        const EsdConv1Args c{in, a[0], blob + h.blob.off[0], h.H, h.W, d.ho[0], d.wo[0], n0};
        const dim3 grid((unsigned)cdiv(d.ho[0] * d.wo[0], D_THREADS), (unsigned)n);
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esd_conv1<true>, grid, dim3(D_THREADS), 0, cx.s, c);
        else hipLaunchKernelGGL(k_esd_conv1<false>, grid, dim3(D_THREADS), 0, cx.s, c);
    })) return rc;
    if (const int rc = esd_conv_launches<64, 128, kEsdPt[1]>(cx, "conv2", a[0], a[1], blob + h.blob.off[1], 1, p, d.ho[0], d.wo[0], N)) return rc;
    if (const int rc = esd_conv_launches<128, 256, kEsdPt[2]>(cx, "conv3", a[1], a[2], blob + h.blob.off[2], 2, p, d.ho[1], d.wo[1], N)) return rc;
    if (const int rc = esd_conv_launches<256, 512, kEsdPt[3]>(cx, "conv4", a[2], a[3], blob + h.blob.off[3], 3, p, d.ho[2], d.wo[2], N)) return rc;
    return cx.launches(N, "fc", [&](int n0, int n) {
        const EsdFcArgs f{a[3], blob + h.blob.fcw, blob + h.blob.fcb, out, (long long)d.features(), n0};
        hipLaunchKernelGGL(k_esd_fc, dim3((unsigned)n), dim3(ESD_FC_THREADS), 0, cx.s, f);
    });
}

// CID_ERR_STATE naming the first layer with a tensor missing.
int esd_all_set(cid_esd_t d, const char* fn) {
    for (int i = 0; i <= kEsdConvs; ++i)
        if (!d->have[i][0] || !d->have[i][1])
            return d->fail(CID_ERR_STATE, std::string(fn) + ": " + (i < kEsdConvs ? kEsdConv[i].name : "fc") + " not set");
    return CID_OK;
}

// The text of CID_ERR_SHAPE for an input that is not the handle's size.
std::string esd_size_message(const cid_esd_s* d, int H, int W) {
    return "input is " + std::to_string(H) + "x" + std::to_string(W) + " but the handle was created for " + std::to_string(d->H) + "x" +
           std::to_string(d->W) + " (the linear layer fixes it)";
}

}  // namespace

extern "C" {

int cid_esd_create(cid_esd_t* out, int H, int W) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (!esd_side_ok(H, W)) return CID_ERR_SHAPE;
    *out = new (std::nothrow) cid_esd_s(H, W);
    return *out ? CID_OK : CID_ERR_INVALID;
}

void cid_esd_destroy(cid_esd_t d) { delete d; }

const char* cid_esd_last_error(cid_esd_t d) { return d ? d->err.c_str() : "null handle"; }

int cid_esd_set_weight(cid_esd_t d, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!d) return CID_ERR_INVALID;
    if (!key || !data || (!shape && ndim > 0)) return d->fail(CID_ERR_INVALID, "cid_esd_set_weight: null argument");
    const std::string k(key);
    int li = -1, is_bias = 0;
    for (int i = 0; i < kEsdConvs; ++i) {
        if (k == std::string(kEsdConv[i].name) + ".weight") { li = i; is_bias = 0; }
        if (k == std::string(kEsdConv[i].name) + ".bias") { li = i; is_bias = 1; }
    }
    if (k == "fc.weight") { li = kEsdFc; is_bias = 0; }
    if (k == "fc.bias") { li = kEsdFc; is_bias = 1; }
    if (li < 0) return d->fail(CID_ERR_KEY, "cid_esd_set_weight: unknown key '" + k + "' (conv1 ... conv4, fc; .weight or .bias)");
    const EsdDims dims(d->H, d->W);
    if (li == kEsdFc) {
        const int64_t F = (int64_t)dims.features();
        const bool ok = is_bias ? (ndim == 1 && shape[0] == 1) : (ndim == 2 && shape[0] == 1 && shape[1] == F);
        if (!ok)
            return d->fail(CID_ERR_SHAPE, "cid_esd_set_weight: size mismatch for " + k + (is_bias ? "" : " (this handle's input gives [1, " +
                                              std::to_string(F) + "])"));
        if (is_bias) {
            d->staging[d->blob.fcb] = data[0];
        } else {
            // reference feature c * P + p (NCHW flatten) -> C8 position ((c / 8) * P + p) * 8 + c % 8
            const size_t P = (size_t)dims.ho[3] * dims.wo[3];
            float* seg = d->staging.data() + d->blob.fcw;
            for (size_t c = 0; c < 512; ++c)
                for (size_t p = 0; p < P; ++p) seg[((c / 8) * P + p) * 8 + c % 8] = data[c * P + p];
        }
        d->have[li][is_bias] = true;
        return CID_OK;
    }
    const auto& L = kEsdConv[li];
    const int64_t want_w[4] = {L.cout, L.cin, 3, 3};
    const bool ok = is_bias ? (ndim == 1 && shape[0] == L.cout) : (ndim == 4 && std::equal(shape, shape + 4, want_w));
    if (!ok) return d->fail(CID_ERR_SHAPE, "cid_esd_set_weight: size mismatch for " + k);
    float* seg = d->staging.data() + d->blob.off[li];
    const size_t nw = (size_t)L.cout * L.cin * 9;
    if (li == 0) std::memcpy(is_bias ? seg + nw : seg, data, (is_bias ? (size_t)L.cout : nw) * sizeof(float));
    else pack_mfma_layer(seg, is_bias ? nullptr : data, is_bias ? data : nullptr, L.cin, L.cout, ESD_PART);
    d->have[li][is_bias] = true;
    return CID_OK;
}

int cid_esd_export_packed(cid_esd_t d, void* host_dst, size_t bytes) {
    if (!d) return CID_ERR_INVALID;
    if (!host_dst) return d->fail(CID_ERR_INVALID, "cid_esd_export_packed: null pointer");
    if (const int rc = esd_all_set(d, "cid_esd_export_packed")) return rc;
    if (bytes < d->blob.total * sizeof(float)) return d->fail(CID_ERR_WORKSPACE, "cid_esd_export_packed: buffer smaller than cid_esd_packed_weights_bytes()");
    std::memcpy(host_dst, d->staging.data(), d->blob.total * sizeof(float));
    return CID_OK;
}

size_t cid_esd_packed_weights_bytes(int H, int W) { return esd_side_ok(H, W) ? EsdBlob(H, W).total * sizeof(float) : 0; }

int cid_esd_upload_weights(cid_esd_t d, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    if (!device_blob) return d->fail(CID_ERR_INVALID, "cid_esd_upload_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return d->fail(CID_ERR_WORKSPACE, "cid_esd_upload_weights: blob must be 256-byte aligned");
    if (const int rc = esd_all_set(d, "cid_esd_upload_weights")) return rc;
    return d->upload_blob("cid_esd_upload_weights: ", device_blob, d->staging.data(), d->blob.total, stream);
}

int cid_esd_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    if (!esd_side_ok(H, W)) return CID_ERR_SHAPE;
    EsdPlan p(H, W);
    return plan_bytes(esd_plan(N, H, W, p), p, bytes);
}

int cid_esd_losses(const float* logit_real, const float* logit_fake, int N, double* out3, void* stream) {
    if (!logit_real || !logit_fake || !out3) return CID_ERR_INVALID;
    if (((uintptr_t)logit_real & 3) || ((uintptr_t)logit_fake & 3) || ((uintptr_t)out3 & 7)) return CID_ERR_INVALID;
    if (N < 1) return CID_ERR_SHAPE;
    const EsdLossArgs a{logit_real, logit_fake, N, out3};
    hipLaunchKernelGGL(k_esd_losses, dim3(1), dim3(D_LOSS_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

int cid_esd_trainer_losses(const float* logit_real, const float* logit_fake, const void* denoised, int d_fmt, const void* clean, int c_fmt,
                           int N, int H, int W, double* out4, void* stream) {
    if (!logit_real || !logit_fake || !denoised || !clean || !out4) return CID_ERR_INVALID;
    if (((uintptr_t)logit_real & 3) || ((uintptr_t)logit_fake & 3) || ((uintptr_t)out4 & 7)) return CID_ERR_INVALID;
    if (!fmt_ok(denoised, d_fmt) || !fmt_ok(clean, c_fmt)) return CID_ERR_INVALID;
    if (N < 1 || !esd_side_ok(H, W)) return CID_ERR_SHAPE;
    const EsdTrainerLossArgs a{{logit_real, logit_fake, N, out4}, denoised, clean, d_fmt, c_fmt, (long long)H * W};
    hipLaunchKernelGGL(k_esd_trainer_losses, dim3(1), dim3(D_LOSS_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
