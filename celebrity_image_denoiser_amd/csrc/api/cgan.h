// The server's CGANGenerator (cid_cg_*): weight staging, BatchNorm folding (pack_bn_fold, esrgan.h), workspace plan and launch
// sequence; kernels in cgan_kernels.h.  Host code.
#pragma once
#include "../cgan_kernels.h"
#include "esrgan.h"

namespace {

constexpr int kCgMaxClasses = 1 << 20;
constexpr int kCgMaxN = 1 << 18;          // every grid and every int index of the kernels stays below 2^31
const int kCgBn[4] = {0, 3, 6, 9};        // model.<i> of the four BatchNorms
const int kCgUp[3] = {2, 5, 8};           // model.<i> of the three transposed convolutions
const int kCgCin[3] = {128, 128, 64}, kCgCout[3] = {128, 64, 32};

std::string cg_layer(int i) { return "model." + std::to_string(i) + "."; }

KeyTable cg_keys(int n_classes) {
    KeyTable k;
    k.tensor("label_emb.weight", {n_classes, CG_LATENT});
    k.tensor("l1.weight", {CG_FEAT, 2 * CG_LATENT});
    k.tensor("l1.bias", {CG_FEAT});
    k.batchnorm(cg_layer(kCgBn[0]), 128);
    for (int u = 0; u < 3; ++u) {
        k.tensor(cg_layer(kCgUp[u]) + "weight", {kCgCin[u], kCgCout[u], 4, 4});
        k.tensor(cg_layer(kCgUp[u]) + "bias", {kCgCout[u]});
        k.batchnorm(cg_layer(kCgBn[u + 1]), kCgCout[u]);
    }
    k.conv("model.11.", 3, 32, 3);
    return k;
}

struct CgPlan {
    size_t l1, t[3], total;   // byte offsets of the C8 tensors: l1's [N,128,8,8] and the three stages' outputs
};

int cg_plan(int N, CgPlan& p) {
    if (N < 1 || N > kCgMaxN) return CID_ERR_SHAPE;
    size_t at = 0;
    p.l1 = take(at, (size_t)N * CG_FEAT * sizeof(float));
    for (int u = 0; u < 3; ++u) p.t[u] = take(at, (size_t)N * kCgCout[u] * (256u << (2 * u)) * sizeof(float));
    p.total = at;
    return CID_OK;
}

}  // namespace

struct cid_cg_s : WeightStore {
    int n_classes = 10;
    double eps[4];
    // the linear, the three stages (weights, bias, s, t), the tail, the embedding table
    size_t up_off(int u) const {
        size_t at = align64(CG_LIN_SEG);
        for (int i = 0; i < u; ++i) at += align64((size_t)16 * kCgCin[i] * kCgCout[i] + 3 * kCgCout[i]);
        return at;
    }
    size_t tail_off() const { return up_off(3); }
    size_t emb_off() const { return tail_off() + CG_TAIL_SEG; }
    size_t blob_floats() const { return emb_off() + align64((size_t)n_classes * CG_LATENT); }
};

namespace {
// The blob from the staged tensors: the kernels' weight layouts, each BatchNorm folded (pack_bn_fold).
void cg_pack(const cid_cg_s* h, float* b) {
    const auto fold = [&](int which, int C, float* s_out, float* t_out) { pack_bn_fold(*h, cg_layer(kCgBn[which]), h->eps[which], C, s_out, t_out); };
    {   // linear: [tile][lane][52]: lane (l16, kq) holds row l16's weights of k = 4 s + kq
        const float *w = h->get("l1.weight"), *bias = h->get("l1.bias");
        for (int tile = 0; tile < CG_LIN_TILES; ++tile)
            for (int row = 0; row < 16; ++row) {
                const int j = cg_lin_feature(tile, row);
                for (int kq = 0; kq < 4; ++kq)
                    for (int s = 0; s < CG_LIN_STEPS; ++s)
                        b[((size_t)tile * 64 + kq * 16 + row) * CG_LIN_LSTR + s] = w[(size_t)j * (2 * CG_LATENT) + 4 * s + kq];
                b[CG_LIN_BIAS + tile * 16 + row] = bias[j];
            }
        fold(0, 128, b + CG_LIN_S, b + CG_LIN_T);
    }
    for (int u = 0; u < 3; ++u) {
        float* seg = b + h->up_off(u);
        const int CI = kCgCin[u], CO = kCgCout[u];
        const float* w = h->get(cg_layer(kCgUp[u]) + "weight");
        for (int ci = 0; ci < CI; ++ci)
            for (int co = 0; co < CO; ++co)
                for (int ky = 0; ky < 4; ++ky)
                    for (int kx = 0; kx < 4; ++kx) seg[cg_up_windex(CO, ci, co, ky, kx)] = w[(((size_t)ci * CO + co) * 4 + ky) * 4 + kx];
        float* tail = seg + (size_t)16 * CI * CO;
        std::memcpy(tail, h->get(cg_layer(kCgUp[u]) + "bias"), CO * sizeof(float));
        fold(u + 1, CO, tail + CO, tail + 2 * CO);
    }
    {   // tail: [ci][tap][co], then the biases
        float* seg = b + h->tail_off();
        const float* w = h->get("model.11.weight");
        for (int co = 0; co < 3; ++co)
            for (int ci = 0; ci < 32; ++ci)
                for (int tap = 0; tap < 9; ++tap) seg[(ci * 9 + tap) * 3 + co] = w[((size_t)co * 32 + ci) * 9 + tap];
        std::memcpy(seg + CG_TAIL_W, h->get("model.11.bias"), 3 * sizeof(float));
    }
    std::memcpy(b + h->emb_off(), h->get("label_emb.weight"), (size_t)h->n_classes * CG_LATENT * sizeof(float));
}
}  // namespace

extern "C" {

int cid_cg_create(cid_cg_t* out, int n_classes) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (n_classes < 1 || n_classes > kCgMaxClasses) return CID_ERR_INVALID;
    cid_cg_s* h = new (std::nothrow) cid_cg_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_cg", cg_keys(n_classes));
    h->n_classes = n_classes;
    std::fill(h->eps, h->eps + 4, 1e-5);
    *out = h;
    return CID_OK;
}

void cid_cg_destroy(cid_cg_t h) { delete h; }

const char* cid_cg_last_error(cid_cg_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_cg_param_key(cid_cg_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_cg_set_weight(cid_cg_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_cg_set_bn_eps(cid_cg_t h, int which, double eps) {
    return h ? h->set_bn_eps(which >= 0 && which <= 3 ? &h->eps[which] : nullptr, eps) : CID_ERR_INVALID;
}

int cid_cg_missing_weights(cid_cg_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_cg_packed_weights_bytes(cid_cg_t h) { return h ? h->blob_floats() * sizeof(float) : 0; }

int cid_cg_upload_weights(cid_cg_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, h->blob_floats(), [h](float* b) { cg_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_cg_workspace_bytes(int N, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    CgPlan p;
    return plan_bytes(cg_plan(N, p), p, bytes);
}

int cid_cg_stage_view(const char* stage, int N, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    CgPlan p;
    const int rc = cg_plan(N, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    int u = -1;
    if (s == "l1") *offset_bytes = p.l1;
    else if (s == "t1") u = 0;
    else if (s == "t2") u = 1;
    else if (s == "t3") u = 2;
    else return CID_ERR_KEY;
    if (u >= 0) *offset_bytes = p.t[u];
    *C = u < 0 ? 128 : kCgCout[u];
    *Hs = *Ws = u < 0 ? 8 : 16 << u;
    *channel_block = 8;
    return CID_OK;
}

int cid_cg_latent(uint64_t seed, uint64_t first_index, int N, float* z_out, void* stream) {
    if (!z_out || ((uintptr_t)z_out & 3)) return CID_ERR_INVALID;
    if (N < 1 || N > kCgMaxN) return CID_ERR_SHAPE;
    const CgLatentArgs a{z_out, (long long)N * CG_LATENT, seed + first_index};
    hipLaunchKernelGGL(k_cg_latent, dim3((unsigned)((a.count + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipPeekAtLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

int cid_cg_forward(cid_cg_t h, const float* z, const int64_t* labels, void* out, int out_fmt, int N, unsigned flags, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_cg_forward", stream);
    if (!z || !labels || !out || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (out_fmt != CID_FMT_F32_NCHW && out_fmt != CID_FMT_U8_NHWC) return cx.fail(CID_ERR_INVALID, "unknown format");
    if (((uintptr_t)z & 3) || ((uintptr_t)labels & 7) || (out_fmt == CID_FMT_F32_NCHW && ((uintptr_t)out & 3)))
        return cx.fail(CID_ERR_INVALID, "misaligned operand");
    if (flags & ~(unsigned)CID_CG_RAW) return cx.fail(CID_ERR_INVALID, "unknown flags");
    if ((flags & CID_CG_RAW) && out_fmt != CID_FMT_F32_NCHW) return cx.fail(CID_ERR_INVALID, "CID_CG_RAW needs an fp32 output");
    CgPlan p;
    if (cg_plan(N, p) != CID_OK) return cx.fail(CID_ERR_SHAPE, "batch size not accepted (1 <= N <= 2^18)");
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_cg_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    const float* blob = h->dev_blob;
    float* l1 = reinterpret_cast<float*>(ws + p.l1);
    float* t[3] = {reinterpret_cast<float*>(ws + p.t[0]), reinterpret_cast<float*>(ws + p.t[1]), reinterpret_cast<float*>(ws + p.t[2])};

    {
        const CgLinearArgs a{z, reinterpret_cast<const long long*>(labels), l1, blob, blob + h->emb_off(), N, h->n_classes};
        hipLaunchKernelGGL(k_cg_linear, dim3(CG_LIN_TILES), dim3(64), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("linear");
    }
    {
        const CgUpArgs a{l1, t[0], blob + h->up_off(0)};
        hipLaunchKernelGGL((k_cg_up<128, 128, 8>), dim3((unsigned)N * CgUpGeom<128, 128, 8>::TILES), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("up 1");
    }
    {
        const CgUpArgs a{t[0], t[1], blob + h->up_off(1)};
        hipLaunchKernelGGL((k_cg_up<128, 64, 16>), dim3((unsigned)N * CgUpGeom<128, 64, 16>::TILES), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("up 2");
    }
    {
        const CgUpArgs a{t[1], t[2], blob + h->up_off(2)};
        hipLaunchKernelGGL((k_cg_up<64, 32, 32>), dim3((unsigned)N * CgUpGeom<64, 32, 32>::TILES), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("up 3");
    }
    {
        const CgTailArgs a{t[2], out, blob + h->tail_off(), (long long)N * 4096};
        const dim3 grid((unsigned)(a.count / D_THREADS));
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_cg_tail<CG_OUT_U8>, grid, dim3(D_THREADS), 0, s, a);
        else if (flags & CID_CG_RAW) hipLaunchKernelGGL(k_cg_tail<CG_OUT_RAW>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_cg_tail<CG_OUT_F32>, grid, dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("tail");
    }
    return CID_OK;
}

}  // extern "C"
