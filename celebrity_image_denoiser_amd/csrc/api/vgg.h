// VGG16 features (cid_vgg_*): LPIPS(net='vgg'), the content loss and its input gradient; kernels in vgg_kernels.h, vgg_bwd_kernels.h
// and lpips_kernels.h; the head pack, the lin keys and kLpMaxN are lpips.h's.  Host code.
#pragma once
#include "../vgg_bwd_kernels.h"
#include "../vgg_kernels.h"
#include "lpips.h"

namespace {

static_assert(VG_MAX_SIDE == CID_VGG_MAX_SIDE, "vgg_kernels.h and cid.h agree on the largest side");
constexpr int kVgMinSide[2] = {16, 4};               // by form: CID_VGG_LPIPS, CID_VGG_CONTENT
const int kVgIdx[VG_CONVS] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};   // torchvision's features indices
const int kVgSlice[VG_CONVS] = {1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5};
const int kVgCin[VG_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kVgCout[VG_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kVgContentConvs = 7;                   // slice1 ... slice3

std::string vg_conv_name(int l) { return "net.slice" + std::to_string(kVgSlice[l]) + "." + std::to_string(kVgIdx[l]) + "."; }

const KeyTable& vg_key_table() {
    static const KeyTable table = [] {
        KeyTable k;
        keys_scaling(k);
        for (int l = 0; l < VG_CONVS; ++l) k.conv(vg_conv_name(l), kVgCout[l], kVgCin[l], 3);
        for (int l = 0; l < LP_TAPS; ++l) k.tensor(lp_lin_name(l), {1, VgTaps::channels(l), 1, 1});
        return k;
    }();
    return table;
}

// blob segments (floats, 64-float aligned): the head, convolutions 1 ... 12 (packed weights then biases), the five lin vectors
size_t vg_conv_off(int l) {   // l = 1 .. 12; l = 13: the lin segment
    size_t at = VG_HEAD_SEG;
    for (int i = 1; i < l; ++i) at += align64((size_t)kVgCout[i] * kVgCin[i] * 9 + kVgCout[i]);
    return at;
}
size_t vg_blob_floats() { return vg_conv_off(VG_CONVS) + VG_LIN_SEG; }

struct VgPlan {
    int Hs[LP_TAPS], Ws[LP_TAPS];    // sizes of relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
    size_t s0, s1;                   // byte offsets of the two scratch tensors (the convolutions between the taps)
    size_t tap[LP_TAPS], total;      // byte offsets of the taps (C8, 2 N images each); the content form has the first three
};

int vg_plan(int what, int N, int H, int W, VgPlan& p) {
    if (what != CID_VGG_LPIPS && what != CID_VGG_CONTENT) return CID_ERR_INVALID;
    if (N < 1 || N > kLpMaxN || H < kVgMinSide[what] || W < kVgMinSide[what] || H > VG_MAX_SIDE || W > VG_MAX_SIDE) return CID_ERR_SHAPE;
    // the head's grid.x runs over the whole batch's pixels
    if (((long long)2 * N * H * W + VG_HEAD_PIX - 1) / VG_HEAD_PIX > 0x7fffffffll) return CID_ERR_SHAPE;
    const int taps = what == CID_VGG_LPIPS ? LP_TAPS : 3;
    p.Hs[0] = H, p.Ws[0] = W;
    for (int k = 1; k < LP_TAPS; ++k) p.Hs[k] = p.Hs[k - 1] / 2, p.Ws[k] = p.Ws[k - 1] / 2;
    for (int k = 0; k < taps; ++k)
        if (vg_stage_bound(p.Hs[k], p.Ws[k]) > (k < 1 ? VG_XPOS_WIDE : LP_XPOS)) return CID_ERR_SHAPE;   // cannot happen up to VG_MAX_SIDE
    size_t at = 0;
    p.s0 = take(at, (size_t)2 * N * 64 * H * W * sizeof(float));
    p.s1 = take(at, (size_t)2 * N * 256 * p.Hs[2] * p.Ws[2] * sizeof(float));
    for (int k = 0; k < LP_TAPS; ++k) {
        p.tap[k] = at;
        if (k < taps) at += align256((size_t)2 * N * VgTaps::channels(k) * p.Hs[k] * p.Ws[k] * sizeof(float));
    }
    p.total = at;
    return CID_OK;
}

// The per-call arena of cid_vgg_content_loss_saved / cid_vgg_content_backward: the seven activations of both towers (2 N images),
// then the seven gradient tensors of tower a (N images), in backward order.
constexpr int kVgSaved = 7;
const char* const kVgActName[kVgSaved] = {"relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3"};
const int kVgActLevel[kVgSaved] = {0, 0, 1, 1, 2, 2, 2};
const char* const kVgGradName[kVgSaved] = {"grad3_3", "grad3_2", "grad3_1", "gradpool2", "grad2_1", "gradpool1", "grad1_1"};
const int kVgGradLevel[kVgSaved] = {2, 2, 2, 2, 1, 1, 0};       // the map size: Hs[level] x Ws[level]
const int kVgGradC[kVgSaved] = {256, 256, 256, 128, 128, 64, 64};

struct VgSavedPlan {
    int Hs[3], Ws[3];
    size_t act[kVgSaved], grad[kVgSaved], total;
};

int vg_saved_plan(int N, int H, int W, VgSavedPlan& p) {
    VgPlan f;
    const int rc = vg_plan(CID_VGG_CONTENT, N, H, W, f);
    if (rc != CID_OK) return rc;
    for (int k = 0; k < 3; ++k) p.Hs[k] = f.Hs[k], p.Ws[k] = f.Ws[k];
    size_t at = 0;
    for (int i = 0; i < kVgSaved; ++i) {
        const int k = kVgActLevel[i];
        p.act[i] = take(at, (size_t)2 * N * VgTaps::channels(k) * p.Hs[k] * p.Ws[k] * sizeof(float));
    }
    for (int i = 0; i < kVgSaved; ++i) {
        const int k = kVgGradLevel[i];
        p.grad[i] = take(at, (size_t)N * kVgGradC[i] * p.Hs[k] * p.Ws[k] * sizeof(float));
    }
    p.total = at;
    return CID_OK;
}

// the backward blob (floats): the head's segment, then the data-gradient weights of convolutions 1 ... 6
size_t vg_bwd_off(int l) {   // l = 1 .. 6; l = 7: the end
    size_t at = VG_HEADB_SEG;
    for (int i = 1; i < l; ++i) at += (size_t)kVgCout[i] * kVgCin[i] * 9;
    return at;
}
size_t vg_bwd_floats() { return vg_bwd_off(kVgContentConvs); }

}  // namespace

struct cid_vgg_s : WeightStore {
    bool full = false;   // the uploaded blob holds all 33 tensors (else slice1 ... slice3 only)
    std::vector<float> bwd_staging;      // the backward blob's staging copy
    const float* dev_bwd = nullptr;      // the uploaded backward blob; dropped when the forward blob is uploaded again
};

namespace {
void vg_pack(const cid_vgg_s* h, float* b, bool full) {
    lp_pack_head(*h, b, vg_conv_name(0), VG_HEAD_K, VG_HEAD_B, VG_HEAD_SS, full);
    for (int l = 1; l < (full ? VG_CONVS : kVgContentConvs); ++l) {
        float* seg = b + vg_conv_off(l);
        const int CO = kVgCout[l], CI = kVgCin[l];
        const float* w = h->get(vg_conv_name(l) + "weight");
        for (int co = 0; co < CO; ++co)
            for (int ci = 0; ci < CI; ++ci)
                for (int t = 0; t < 9; ++t) seg[lp_conv_windex(CI, 3, co, ci, t / 3, t % 3)] = w[((size_t)co * CI + ci) * 9 + t];
        std::memcpy(seg + (size_t)CO * CI * 9, h->get(vg_conv_name(l) + "bias"), CO * sizeof(float));
    }
    if (full)
        for (int l = 0; l < LP_TAPS; ++l)
            std::memcpy(b + vg_conv_off(VG_CONVS) + VgTaps::lin_off(l), h->get(lp_lin_name(l)), VgTaps::channels(l) * sizeof(float));
}

// The data gradient of a 3x3, pad-1, stride-1 convolution is a 3x3 convolution with the channel axes swapped and the taps flipped:
// w'[ci][co][kh][kw] = w[co][ci][2 - kh][2 - kw], packed with lp_conv_windex like a forward convolution of co -> ci channels.
void vg_pack_backward(const cid_vgg_s* h, float* b) {
    const float* w0 = h->get(vg_conv_name(0) + "weight");
    for (int t = 0; t < 9; ++t)
        for (int co = 0; co < 64; ++co)
            for (int ci = 0; ci < 3; ++ci) b[(t * 64 + co) * 3 + ci] = w0[(co * 3 + ci) * 9 + (2 - t / 3) * 3 + (2 - t % 3)];
    for (int l = 1; l < kVgContentConvs; ++l) {
        float* seg = b + vg_bwd_off(l);
        const int CG = kVgCout[l], CX = kVgCin[l];
        const float* w = h->get(vg_conv_name(l) + "weight");
        for (int cx = 0; cx < CX; ++cx)
            for (int cg = 0; cg < CG; ++cg)
                for (int t = 0; t < 9; ++t) seg[lp_conv_windex(CG, 3, cx, cg, t / 3, t % 3)] = w[((size_t)cg * CX + cx) * 9 + (8 - t)];
    }
}

// One trunk convolution from an Hs x Ws tensor; the plane size follows the output map's width.  Only the launch that can meet a
// map wider than 339 (relu1_2, at the image's own size) has a wide instantiation.
template <int CIN, int COUT, bool POOL, bool CAN_BE_WIDE>
void vg_conv_launch(const float* in, float* out, const float* w, int N, int Hs, int Ws, hipStream_t s) {
    const int Ho = POOL ? Hs / 2 : Hs, Wo = POOL ? Ws / 2 : Ws;
    const LpConvArgs a{in, out, w, (long long)2 * N * Ho * Wo, Hs, Ws, Ho, Wo};
    const dim3 grid((unsigned)((a.total + LP_NT - 1) / LP_NT), COUT / LP_MT);
    if (vg_stage_bound(Ho, Wo) <= LP_XPOS) {
        hipLaunchKernelGGL((k_lpips_conv<CIN, COUT, 3, POOL, 2, LP_XPOS>), grid, dim3(D_THREADS), 0, s, a);
    } else if constexpr (CAN_BE_WIDE) {
        hipLaunchKernelGGL((k_lpips_conv<CIN, COUT, 3, POOL, 2, VG_XPOS_WIDE>), grid, dim3(D_THREADS), 0, s, a);
    }
}

// the checks cid_vgg_lpips and cid_vgg_content_loss share
int vg_check(const Call& cx, int what, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags,
             const void* out, const void* layers, const void* workspace, size_t workspace_bytes, VgPlan& p, bool saved = false) {
    if (!a || !b || !out || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if ((fmt_a != CID_FMT_F32_NCHW && fmt_a != CID_FMT_U8_NHWC) || (fmt_b != CID_FMT_F32_NCHW && fmt_b != CID_FMT_U8_NHWC))
        return cx.fail(CID_ERR_INVALID, "unknown format");
    if (saved && fmt_a != CID_FMT_F32_NCHW) return cx.fail(CID_ERR_INVALID, "operand a must be fp32 (a uint8 image has no gradient)");
    if ((fmt_a == CID_FMT_F32_NCHW && ((uintptr_t)a & 3)) || (fmt_b == CID_FMT_F32_NCHW && ((uintptr_t)b & 3)) || ((uintptr_t)out & 7) ||
        ((uintptr_t)layers & 7))
        return cx.fail(CID_ERR_INVALID, "misaligned operand");
    if (flags & ~(unsigned)CID_LPIPS_UNIT_VIEW) return cx.fail(CID_ERR_INVALID, "unknown flags");
    if (vg_plan(what, N, H, W, p) != CID_OK)
        return cx.fail(CID_ERR_SHAPE, std::string("shape not accepted (1 <= N <= 2^20, ") + std::to_string(kVgMinSide[what]) + " <= H, W <= " +
                                            std::to_string(VG_MAX_SIDE) + ", 2 N H W < 2^37)");
    VgSavedPlan sp;
    if (saved) vg_saved_plan(N, H, W, sp);
    if (const int rc = saved ? cx.room(workspace, workspace_bytes, sp.total, "cid_vgg_saved_bytes", "saved arena")
                             : cx.room(workspace, workspace_bytes, p.total, "cid_vgg_workspace_bytes"))
        return rc;
    if (const int rc = cx.uploaded()) return rc;
    return CID_OK;
}

// Head and trunk up to convolution `convs` (7: relu3_3, 13: relu5_3); convolution l writes t[l], every tensor C8 with 2 N images, and
// Hs / Ws are the sizes by level (the image's, then one halving per pool).  The plain calls pass their two scratch tensors and the
// taps, the saved call seven tensors of its arena: the same kernels on the same operands, so the same bits.  Returns the name of the
// launch that failed, or null.
const char* vg_features(cid_vgg_t h, float* const* t, const int* Hs, const int* Ws, const void* a, int fmt_a, const void* b, int fmt_b, int N,
                        int H, int W, bool unit, bool scaled, int convs, hipStream_t s) {
    const float* blob = h->dev_blob;
    {
        const VgHeadArgs ha{a, b, t[0], blob, (long long)2 * N * H * W, H, W, N, fmt_a == CID_FMT_U8_NHWC, fmt_b == CID_FMT_U8_NHWC, unit, scaled};
        hipLaunchKernelGGL(k_vgg_head, dim3((unsigned)((ha.total + VG_HEAD_PIX - 1) / VG_HEAD_PIX)), dim3(VG_HEAD_PIX), 0, s, ha);
        if (hipPeekAtLastError() != hipSuccess) return "relu1_1";
    }
    vg_conv_launch<64, 64, false, true>(t[0], t[1], blob + vg_conv_off(1), N, Hs[0], Ws[0], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu1_2";
    vg_conv_launch<64, 128, true, false>(t[1], t[2], blob + vg_conv_off(2), N, Hs[0], Ws[0], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu2_1";
    vg_conv_launch<128, 128, false, false>(t[2], t[3], blob + vg_conv_off(3), N, Hs[1], Ws[1], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu2_2";
    vg_conv_launch<128, 256, true, false>(t[3], t[4], blob + vg_conv_off(4), N, Hs[1], Ws[1], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu3_1";
    vg_conv_launch<256, 256, false, false>(t[4], t[5], blob + vg_conv_off(5), N, Hs[2], Ws[2], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu3_2";
    vg_conv_launch<256, 256, false, false>(t[5], t[6], blob + vg_conv_off(6), N, Hs[2], Ws[2], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu3_3";
    if (convs == kVgContentConvs) return nullptr;
    vg_conv_launch<256, 512, true, false>(t[6], t[7], blob + vg_conv_off(7), N, Hs[2], Ws[2], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu4_1";
    vg_conv_launch<512, 512, false, false>(t[7], t[8], blob + vg_conv_off(8), N, Hs[3], Ws[3], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu4_2";
    vg_conv_launch<512, 512, false, false>(t[8], t[9], blob + vg_conv_off(9), N, Hs[3], Ws[3], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu4_3";
    vg_conv_launch<512, 512, true, false>(t[9], t[10], blob + vg_conv_off(10), N, Hs[3], Ws[3], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu5_1";
    vg_conv_launch<512, 512, false, false>(t[10], t[11], blob + vg_conv_off(11), N, Hs[4], Ws[4], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu5_2";
    vg_conv_launch<512, 512, false, false>(t[11], t[12], blob + vg_conv_off(12), N, Hs[4], Ws[4], s);
    if (hipPeekAtLastError() != hipSuccess) return "relu5_3";
    return nullptr;
}

// the plain calls' tensors by convolution: the two scratch tensors between the taps
void vg_plain_tensors(const VgPlan& p, char* ws, float** t) {
    float *s0 = reinterpret_cast<float*>(ws + p.s0), *s1 = reinterpret_cast<float*>(ws + p.s1), *tap[LP_TAPS];
    for (int k = 0; k < LP_TAPS; ++k) tap[k] = reinterpret_cast<float*>(ws + p.tap[k]);
    float* const by_conv[VG_CONVS] = {s0, tap[0], s0, tap[1], s0, s1, tap[2], s0, s1, tap[3], s0, s1, tap[4]};
    std::copy(by_conv, by_conv + VG_CONVS, t);
}

// One data-gradient launch over tower a's N images of an Ho x Wo map; the plane size follows the map's width, as in vg_conv_launch.
template <int CG, int CX, bool UNPOOL, bool MASK, bool CAN_BE_WIDE>
void vg_dgrad_launch(const float* g, const float* pool, const float* act, float* out, const float* w, int N, int Ho, int Wo, hipStream_t s) {
    const VgDgradArgs a{g, pool, act, out, w, (long long)N * Ho * Wo, Ho, Wo};
    const dim3 grid((unsigned)((a.total + LP_NT - 1) / LP_NT), CX / LP_MT);
    if (vg_stage_bound(Ho, Wo) <= LP_XPOS) {
        hipLaunchKernelGGL((k_vgg_dgrad<CG, CX, UNPOOL, MASK, LP_XPOS>), grid, dim3(D_THREADS), 0, s, a);
    } else if constexpr (CAN_BE_WIDE) {
        hipLaunchKernelGGL((k_vgg_dgrad<CG, CX, UNPOOL, MASK, VG_XPOS_WIDE>), grid, dim3(D_THREADS), 0, s, a);
    }
}
}  // namespace

extern "C" {

int cid_vgg_create(cid_vgg_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    cid_vgg_s* h = new (std::nothrow) cid_vgg_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_vgg", vg_key_table());
    *out = h;
    return CID_OK;
}

void cid_vgg_destroy(cid_vgg_t h) { delete h; }

const char* cid_vgg_last_error(cid_vgg_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_vgg_param_key(cid_vgg_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_vgg_set_weight(cid_vgg_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_vgg_missing_weights(cid_vgg_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_vgg_packed_weights_bytes(cid_vgg_t h) { return h ? vg_blob_floats() * sizeof(float) : 0; }

int cid_vgg_upload_weights(cid_vgg_t h, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!device_blob) return h->fail(CID_ERR_INVALID, "cid_vgg_upload_weights: null device pointer");
    // all 33 tensors, or exactly the 14 of slice1 ... slice3 (key table entries 2 ... 15); this state check comes ahead of the
    // blob's alignment check, which the shared upload makes
    int set = 0, content = 0;
    for (size_t i = 0; i < h->have.size(); ++i) {
        set += h->have[i] != 0;
        content += h->have[i] && i >= 2 && i < 2 + 2 * (size_t)kVgContentConvs;
    }
    const bool full = set == CID_VGG_NUM_WEIGHTS;
    if (!full && !(set == 2 * kVgContentConvs && content == set))
        return h->fail(CID_ERR_STATE, "cid_vgg_upload_weights: needs all " + std::to_string(CID_VGG_NUM_WEIGHTS) +
                                          " tensors or exactly the 14 of slice1 ... slice3; " + std::to_string(set) + " set, first missing " +
                                          h->keys[h->first_missing()].name);
    const int rc = h->upload(device_blob, stream, vg_blob_floats(), [h, full](float* b) { vg_pack(h, b, full); }, false);
    if (rc == CID_OK) {
        h->full = full;
        h->dev_bwd = nullptr;   // packed from the previous weights
    }
    return rc;
}

int cid_vgg_workspace_bytes(int what, int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    VgPlan p;
    return plan_bytes(vg_plan(what, N, H, W, p), p, bytes);
}

int cid_vgg_stage_view(int what, const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    VgPlan p;
    const int rc = vg_plan(what, N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    if (s.size() != 5 || s.compare(0, 4, "relu") != 0 || s[4] < '1' || s[4] > (what == CID_VGG_LPIPS ? '5' : '3')) return CID_ERR_KEY;
    const int k = s[4] - '1';
    *offset_bytes = p.tap[k];
    *C = VgTaps::channels(k);
    *Hs = p.Hs[k];
    *Ws = p.Ws[k];
    *channel_block = 8;
    return CID_OK;
}

int cid_vgg_lpips(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
                  double* layers, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_vgg_lpips", stream);
    VgPlan p;
    if (const int rc = vg_check(cx, CID_VGG_LPIPS, a, fmt_a, b, fmt_b, N, H, W, flags, out, layers, workspace, workspace_bytes, p)) return rc;
    if (!h->full) return cx.fail(CID_ERR_STATE, "the handle holds slice1 ... slice3 only (content loss)");
    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    float* t[VG_CONVS];
    vg_plain_tensors(p, ws, t);
    if (const char* failed = vg_features(h, t, p.Hs, p.Ws, a, fmt_a, b, fmt_b, N, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0, true, VG_CONVS, s))
        return cx.hip(failed);
    LpDistArgs da;
    for (int k = 0; k < LP_TAPS; ++k) {
        da.tap[k] = reinterpret_cast<const float*>(ws + p.tap[k]);
        da.P[k] = p.Hs[k] * p.Ws[k];
    }
    da.lin = h->dev_blob + vg_conv_off(VG_CONVS);
    da.out = out;
    da.layers = layers;
    da.N = N;
    hipLaunchKernelGGL(k_lpips_dist<VgTaps>, dim3((unsigned)N), dim3(D_THREADS), 0, s, da);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("distance");
    return CID_OK;
}

int cid_vgg_content_loss(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_vgg_content_loss", stream);
    VgPlan p;
    if (const int rc = vg_check(cx, CID_VGG_CONTENT, a, fmt_a, b, fmt_b, N, H, W, flags, out, nullptr, workspace, workspace_bytes, p)) return rc;
    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    float* t[VG_CONVS];
    vg_plain_tensors(p, ws, t);
    if (const char* failed = vg_features(h, t, p.Hs, p.Ws, a, fmt_a, b, fmt_b, N, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0, false, kVgContentConvs, s))
        return cx.hip(failed);
    const VgContentArgs ca{reinterpret_cast<const float*>(ws + p.tap[2]), out, (long long)256 * p.Hs[2] * p.Ws[2], N};
    hipLaunchKernelGGL(k_vgg_content, dim3((unsigned)N), dim3(D_THREADS), 0, s, ca);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("loss");
    return CID_OK;
}

int cid_vgg_saved_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    VgSavedPlan p;
    return plan_bytes(vg_saved_plan(N, H, W, p), p, bytes);
}

int cid_vgg_saved_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* images, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !images || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    VgSavedPlan p;
    const int rc = vg_saved_plan(N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    for (int i = 0; i < kVgSaved; ++i) {
        const bool act = s == kVgActName[i];
        if (!act && s != kVgGradName[i]) continue;
        const int k = act ? kVgActLevel[i] : kVgGradLevel[i];
        *offset_bytes = act ? p.act[i] : p.grad[i];
        *images = act ? 2 * N : N;
        *C = act ? VgTaps::channels(k) : kVgGradC[i];
        *Hs = p.Hs[k];
        *Ws = p.Ws[k];
        *channel_block = 8;
        return CID_OK;
    }
    return CID_ERR_KEY;
}

int cid_vgg_content_loss_saved(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags,
                               double* out, void* saved, size_t saved_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_vgg_content_loss_saved", stream);
    VgPlan fp;
    if (const int rc = vg_check(cx, CID_VGG_CONTENT, a, fmt_a, b, fmt_b, N, H, W, flags, out, nullptr, saved, saved_bytes, fp, true)) return rc;
    VgSavedPlan p;
    vg_saved_plan(N, H, W, p);
    const hipStream_t s = cx.s;
    char* sv = static_cast<char*>(saved);
    float* t[kVgSaved];
    for (int i = 0; i < kVgSaved; ++i) t[i] = reinterpret_cast<float*>(sv + p.act[i]);
    if (const char* failed = vg_features(h, t, p.Hs, p.Ws, a, fmt_a, b, fmt_b, N, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0, false, kVgContentConvs, s))
        return cx.hip(failed);
    const VgContentArgs ca{t[6], out, (long long)256 * p.Hs[2] * p.Ws[2], N};
    hipLaunchKernelGGL(k_vgg_content, dim3((unsigned)N), dim3(D_THREADS), 0, s, ca);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("loss");
    return CID_OK;
}

size_t cid_vgg_backward_weights_bytes(cid_vgg_t h) { return h ? vg_bwd_floats() * sizeof(float) : 0; }

int cid_vgg_upload_backward_weights(cid_vgg_t h, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const std::string fn = "cid_vgg_upload_backward_weights: ";
    if (!device_blob) return h->fail(CID_ERR_INVALID, fn + "null device pointer");
    for (int i = 2; i < 2 + 2 * kVgContentConvs; ++i)
        if (!h->have[i]) return h->fail(CID_ERR_STATE, fn + h->keys[i].name + " not set");
    if ((uintptr_t)device_blob & 255) return h->fail(CID_ERR_WORKSPACE, fn + "blob must be 256-byte aligned");
    h->bwd_staging.assign(vg_bwd_floats(), 0.f);
    vg_pack_backward(h, h->bwd_staging.data());
    return h->upload_blob(fn, device_blob, h->bwd_staging.data(), h->bwd_staging.size(), stream, &h->dev_bwd);
}

int cid_vgg_content_backward(cid_vgg_t h, const double* grad_out, float* grad_a, int N, int H, int W, unsigned flags, void* saved,
                             size_t saved_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_vgg_content_backward", stream);
    if (!grad_out || !grad_a || !saved) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (((uintptr_t)grad_out & 7) || ((uintptr_t)grad_a & 3)) return cx.fail(CID_ERR_INVALID, "misaligned operand");
    if (flags & ~(unsigned)CID_LPIPS_UNIT_VIEW) return cx.fail(CID_ERR_INVALID, "unknown flags");
    VgSavedPlan p;
    if (vg_saved_plan(N, H, W, p) != CID_OK)
        return cx.fail(CID_ERR_SHAPE, std::string("shape not accepted (1 <= N <= 2^20, 4 <= H, W <= ") + std::to_string(VG_MAX_SIDE) + ", 2 N H W < 2^37)");
    if (const int rc = cx.room(saved, saved_bytes, p.total, "cid_vgg_saved_bytes", "saved arena")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    if (!h->dev_bwd) return cx.fail(CID_ERR_STATE, "backward weights not uploaded (cid_vgg_upload_backward_weights)");
    const hipStream_t s = cx.s;
    char* sv = static_cast<char*>(saved);
    const float* act[kVgSaved];
    float* g[kVgSaved];
    for (int i = 0; i < kVgSaved; ++i) {
        act[i] = reinterpret_cast<const float*>(sv + p.act[i]);
        g[i] = reinterpret_cast<float*>(sv + p.grad[i]);
    }
    const float* bw = h->dev_bwd;
    const int H1 = p.Hs[0], W1 = p.Ws[0], H2 = p.Hs[1], W2 = p.Ws[1], H3 = p.Hs[2], W3 = p.Ws[2];
    {
        VgSeedArgs sa{act[6], grad_out, g[0], (long long)256 * H3 * W3, 0, N};
        sa.total = sa.count * N;
        hipLaunchKernelGGL(k_vgg_seed, dim3((unsigned)((sa.total / 4 + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, s, sa);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("grad3_3");
    }
    vg_dgrad_launch<256, 256, false, true, false>(g[0], nullptr, act[5], g[1], bw + vg_bwd_off(6), N, H3, W3, s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("grad3_2");
    vg_dgrad_launch<256, 256, false, true, false>(g[1], nullptr, act[4], g[2], bw + vg_bwd_off(5), N, H3, W3, s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("grad3_1");
    vg_dgrad_launch<256, 128, false, false, false>(g[2], nullptr, nullptr, g[3], bw + vg_bwd_off(4), N, H3, W3, s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("gradpool2");
    vg_dgrad_launch<128, 128, true, true, false>(g[3], act[3], act[2], g[4], bw + vg_bwd_off(3), N, H2, W2, s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("grad2_1");
    vg_dgrad_launch<128, 64, false, false, false>(g[4], nullptr, nullptr, g[5], bw + vg_bwd_off(2), N, H2, W2, s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("gradpool1");
    vg_dgrad_launch<64, 64, true, true, true>(g[5], act[1], act[0], g[6], bw + vg_bwd_off(1), N, H1, W1, s);
    if (hipPeekAtLastError() != hipSuccess) return cx.hip("grad1_1");
    {
        const VgHeadBwdArgs ha{g[6], grad_a, bw, (long long)N * H * W, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0};
        hipLaunchKernelGGL(k_vgg_head_bwd, dim3((unsigned)((ha.total + VG_HEAD_PIX - 1) / VG_HEAD_PIX)), dim3(VG_HEAD_PIX), 0, s, ha);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("grad_a");
    }
    return CID_OK;
}

}  // extern "C"
