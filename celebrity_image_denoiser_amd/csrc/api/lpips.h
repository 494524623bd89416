// LPIPS(net='alex') (cid_lpips_*): weight staging, workspace plan and launch sequence; kernels in lpips_kernels.h.  pack_k64 is
// esrgan.h's.  Host code.
#pragma once
#include "../lpips_kernels.h"
#include "esrgan.h"

namespace {

constexpr int kLpMaxN = 1 << 20;
constexpr int kLpMinSide = 31;
const int kLpSlice[5] = {0, 3, 6, 8, 10};            // net.slice<k+1>.<i>
const int kLpCin[5] = {3, 64, 192, 384, 256}, kLpKs[5] = {11, 5, 3, 3, 3};

// scaling_layer.* ahead of a tower's convolutions, lin<k>.* behind them: the layout LPIPS and the VGG tower share
void keys_scaling(KeyTable& k) {
    k.tensor("scaling_layer.shift", {1, 3, 1, 1});
    k.tensor("scaling_layer.scale", {1, 3, 1, 1});
}
std::string lp_lin_name(int l) { return "lin" + std::to_string(l) + ".model.1.weight"; }
std::string lp_conv_name(int l) { return "net.slice" + std::to_string(l + 1) + "." + std::to_string(kLpSlice[l]) + "."; }

const KeyTable& lp_key_table() {
    static const KeyTable table = [] {
        KeyTable k;
        keys_scaling(k);
        for (int l = 0; l < LP_TAPS; ++l) k.conv(lp_conv_name(l), lp_channels(l), kLpCin[l], kLpKs[l]);
        for (int l = 0; l < LP_TAPS; ++l) k.tensor(lp_lin_name(l), {1, lp_channels(l), 1, 1});
        return k;
    }();
    return table;
}

// blob segments (floats, 64-float aligned): the head, relu2 ... relu5 (packed weights then biases), the five lin vectors
size_t lp_conv_off(int l) {   // l = 1 .. 4; l = 5: the lin segment
    size_t at = LP_HEAD_SEG;
    for (int i = 1; i < l; ++i) at += align64((size_t)lp_channels(i) * kLpCin[i] * kLpKs[i] * kLpKs[i] + lp_channels(i));
    return at;
}
size_t lp_blob_floats() { return lp_conv_off(5) + LP_LIN_SEG; }

struct LpPlan {
    int Hs[LP_TAPS], Ws[LP_TAPS];   // sizes of relu1 ... relu5
    size_t tap[LP_TAPS], total;     // byte offsets of the C8 tensors (2 N images each)
};

int lp_plan(int N, int H, int W, LpPlan& p) {
    if (N < 1 || N > kLpMaxN || H < kLpMinSide || W < kLpMinSide || (long long)H * W >= (1ll << 31)) return CID_ERR_SHAPE;
    p.Hs[0] = (H - 7) / 4 + 1, p.Ws[0] = (W - 7) / 4 + 1;
    p.Hs[1] = (p.Hs[0] - 3) / 2 + 1, p.Ws[1] = (p.Ws[0] - 3) / 2 + 1;
    p.Hs[2] = (p.Hs[1] - 3) / 2 + 1, p.Ws[2] = (p.Ws[1] - 3) / 2 + 1;
    p.Hs[3] = p.Hs[4] = p.Hs[2], p.Ws[3] = p.Ws[4] = p.Ws[2];
    // what a workgroup of the GEMM kernel stages must fit its LDS planes
    if (lp_stage_bound(p.Hs[1], p.Ws[1], 2) > LP_XPOS || lp_stage_bound(p.Hs[2], p.Ws[2], 1) > LP_XPOS) return CID_ERR_SHAPE;
    size_t at = 0;
    for (int k = 0; k < LP_TAPS; ++k) p.tap[k] = take(at, (size_t)2 * N * lp_channels(k) * p.Hs[k] * p.Ws[k] * sizeof(float));
    p.total = at;
    return CID_OK;
}

}  // namespace

struct cid_lpips_s : WeightStore {};

namespace {
// A tower's head segment: [k][64], bias, and (scaled) the scaling layer's shift and scale
void lp_pack_head(const WeightStore& w, float* b, const std::string& conv, int K, int bias_at, int ss_at, bool scaled) {
    pack_k64(b, w.get(conv + "weight"), K);
    std::memcpy(b + bias_at, w.get(conv + "bias"), 64 * sizeof(float));
    if (!scaled) return;
    std::memcpy(b + ss_at, w.get("scaling_layer.shift"), 3 * sizeof(float));
    std::memcpy(b + ss_at + 4, w.get("scaling_layer.scale"), 3 * sizeof(float));
}

void lp_pack(const cid_lpips_s* h, float* b) {
    lp_pack_head(*h, b, lp_conv_name(0), LP_HEAD_K, LP_HEAD_B, LP_HEAD_SS, true);
    for (int l = 1; l < LP_TAPS; ++l) {
        float* seg = b + lp_conv_off(l);
        const int CO = lp_channels(l), CI = kLpCin[l], KS = kLpKs[l];
        const float* w = h->get(lp_conv_name(l) + "weight");
        for (int co = 0; co < CO; ++co)
            for (int ci = 0; ci < CI; ++ci)
                for (int kh = 0; kh < KS; ++kh)
                    for (int kw = 0; kw < KS; ++kw) seg[lp_conv_windex(CI, KS, co, ci, kh, kw)] = w[(((size_t)co * CI + ci) * KS + kh) * KS + kw];
        std::memcpy(seg + (size_t)CO * CI * KS * KS, h->get(lp_conv_name(l) + "bias"), CO * sizeof(float));
    }
    for (int l = 0; l < LP_TAPS; ++l) std::memcpy(b + lp_conv_off(5) + lp_lin_off(l), h->get(lp_lin_name(l)), lp_channels(l) * sizeof(float));
}

template <int CIN, int COUT, int KS, bool POOL>
void lp_conv_launch(const float* in, float* out, const float* w, int N, int Hs, int Ws, int Ho, int Wo, hipStream_t s) {
    const LpConvArgs a{in, out, w, (long long)2 * N * Ho * Wo, Hs, Ws, Ho, Wo};
    const dim3 grid((unsigned)((a.total + LP_NT - 1) / LP_NT), COUT / LP_MT);
    hipLaunchKernelGGL((k_lpips_conv<CIN, COUT, KS, POOL>), grid, dim3(D_THREADS), 0, s, a);
}
}  // namespace

extern "C" {

int cid_lpips_create(cid_lpips_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    cid_lpips_s* h = new (std::nothrow) cid_lpips_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_lpips", lp_key_table());
    *out = h;
    return CID_OK;
}

void cid_lpips_destroy(cid_lpips_t h) { delete h; }

const char* cid_lpips_last_error(cid_lpips_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_lpips_param_key(cid_lpips_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_lpips_set_weight(cid_lpips_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_lpips_missing_weights(cid_lpips_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_lpips_packed_weights_bytes(cid_lpips_t h) { return h ? lp_blob_floats() * sizeof(float) : 0; }

int cid_lpips_upload_weights(cid_lpips_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, lp_blob_floats(), [h](float* b) { lp_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_lpips_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    LpPlan p;
    return plan_bytes(lp_plan(N, H, W, p), p, bytes);
}

int cid_lpips_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    LpPlan p;
    const int rc = lp_plan(N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    if (s.size() != 5 || s.compare(0, 4, "relu") != 0 || s[4] < '1' || s[4] > '5') return CID_ERR_KEY;
    const int k = s[4] - '1';
    *offset_bytes = p.tap[k];
    *C = lp_channels(k);
    *Hs = p.Hs[k];
    *Ws = p.Ws[k];
    *channel_block = 8;
    return CID_OK;
}

int cid_lpips(cid_lpips_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
              double* layers, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_lpips", stream);
    if (!a || !b || !out || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if ((fmt_a != CID_FMT_F32_NCHW && fmt_a != CID_FMT_U8_NHWC) || (fmt_b != CID_FMT_F32_NCHW && fmt_b != CID_FMT_U8_NHWC))
        return cx.fail(CID_ERR_INVALID, "unknown format");
    if ((fmt_a == CID_FMT_F32_NCHW && ((uintptr_t)a & 3)) || (fmt_b == CID_FMT_F32_NCHW && ((uintptr_t)b & 3)) || ((uintptr_t)out & 7) ||
        ((uintptr_t)layers & 7))
        return cx.fail(CID_ERR_INVALID, "misaligned operand");
    if (flags & ~(unsigned)CID_LPIPS_UNIT_VIEW) return cx.fail(CID_ERR_INVALID, "unknown flags");
    LpPlan p;
    if (lp_plan(N, H, W, p) != CID_OK)
        return cx.fail(CID_ERR_SHAPE, "shape not accepted (1 <= N <= 2^20, H and W >= 31 and within the kernels' tile limit)");
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_lpips_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    const float* blob = h->dev_blob;
    float* t[LP_TAPS];
    for (int k = 0; k < LP_TAPS; ++k) t[k] = reinterpret_cast<float*>(ws + p.tap[k]);

    if (const int rc = cx.launches(2ll * N, "head", [&](int n0, int n) {   // both towers: 2 N images
        const LpHeadArgs ha{a, b, t[0], blob, H, W, p.Hs[0], p.Ws[0], N, n0, fmt_a == CID_FMT_U8_NHWC, fmt_b == CID_FMT_U8_NHWC,
                            (flags & CID_LPIPS_UNIT_VIEW) != 0};
        const dim3 grid((unsigned)((p.Hs[0] * p.Ws[0] + LP_HEAD_PIX - 1) / LP_HEAD_PIX), (unsigned)n);
        hipLaunchKernelGGL(k_lpips_head, grid, dim3(LP_HEAD_PIX), 0, s, ha);
    })) return rc;
    lp_conv_launch<64, 192, 5, true>(t[0], t[1], blob + lp_conv_off(1), N, p.Hs[0], p.Ws[0], p.Hs[1], p.Ws[1], s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("relu2");
    lp_conv_launch<192, 384, 3, true>(t[1], t[2], blob + lp_conv_off(2), N, p.Hs[1], p.Ws[1], p.Hs[2], p.Ws[2], s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("relu3");
    lp_conv_launch<384, 256, 3, false>(t[2], t[3], blob + lp_conv_off(3), N, p.Hs[2], p.Ws[2], p.Hs[3], p.Ws[3], s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("relu4");
    lp_conv_launch<256, 256, 3, false>(t[3], t[4], blob + lp_conv_off(4), N, p.Hs[3], p.Ws[3], p.Hs[4], p.Ws[4], s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("relu5");
    {
        LpDistArgs da;
        for (int k = 0; k < LP_TAPS; ++k) {
            da.tap[k] = t[k];
            da.P[k] = p.Hs[k] * p.Ws[k];
        }
        da.lin = blob + lp_conv_off(5);
        da.out = out;
        da.layers = layers;
        da.N = N;
        hipLaunchKernelGGL(k_lpips_dist<LpAlexTaps>, dim3((unsigned)N), dim3(D_THREADS), 0, s, da);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("distance");
    }
    return CID_OK;
}

}  // extern "C"
