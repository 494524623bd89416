// The server's ESRGANGenerator (cid_esr_*): weight staging, BatchNorm folding, workspace plan and launch sequence; kernels in
// esrgan_kernels.h (its tiles are DiscGeom's, disc_kernels.h).  Host code.
#pragma once
#include "../disc_kernels.h"
#include "../esrgan_kernels.h"
#include "../weight_store.h"

namespace {

constexpr int kEsrMaxBlocks = CID_ESR_MAX_RESIDUALS;
constexpr size_t kEsrHeadSeg = (size_t)E_HEAD_K * 64 + 128;      // weights, bias[64], slope (padded to 64)
constexpr size_t kEsrConvSeg = (size_t)E_CONV_W + 256;           // weights, bias[64], s[64], t[64], slope (padded to 64)
constexpr size_t kEsrTailSeg = (size_t)E_TAIL_W + 64;            // weights, bias[3] (padded to 64)

// The key tables and pack steps below stand on WeightStore (weight_store.h).  What SRGAN shares with ESRGAN is written once here.
void keys_head9(KeyTable& k) {
    k.conv("initial.0.", 64, 3, 9);
    k.tensor("initial.1.weight", {1});
}

// <blk>0 conv, <blk>1 BatchNorm, <blk>2 PReLU, <blk>3 conv, <blk>4 BatchNorm
void keys_res_block(KeyTable& k, const std::string& blk) {
    for (int c = 0; c < 2; ++c) {
        k.conv(blk + std::to_string(3 * c) + ".", 64, 64, 3);
        k.batchnorm(blk + std::to_string(3 * c + 1) + ".", 64);
        if (c == 0) k.tensor(blk + "2.weight", {1});
    }
}

KeyTable esr_keys(int R) {
    KeyTable k;
    keys_head9(k);
    for (int i = 0; i < R; ++i) keys_res_block(k, "residuals." + std::to_string(i) + ".block.");
    k.conv("final.", 3, 64, 9);
    return k;
}

// The BatchNorm under the key prefix `bn` folded to y = s*z + t with s = gamma / sqrt(running_var + eps), t = beta - running_mean * s,
// derived in fp64 and rounded once to fp32.
void pack_bn_fold(const WeightStore& w, const std::string& bn, double eps, int C, float* s_out, float* t_out) {
    const float *gamma = w.get(bn + "weight"), *beta = w.get(bn + "bias"), *mean = w.get(bn + "running_mean"), *var = w.get(bn + "running_var");
    for (int ch = 0; ch < C; ++ch) {
        const double s = (double)gamma[ch] / std::sqrt((double)var[ch] + eps);
        s_out[ch] = (float)s;
        t_out[ch] = (float)((double)beta[ch] - (double)mean[ch] * s);
    }
}

// A 64-channel convolution's [co][K] weights as the [k][64] rows a head kernel reads.
void pack_k64(float* dst, const float* w, int K) {
    for (int co = 0; co < 64; ++co)
        for (int k = 0; k < K; ++k) dst[(size_t)k * 64 + co] = w[(size_t)co * K + k];
}

// initial.*, the 9x9 head: [ci][kh][kw][co], bias, the PReLU's slope
void pack_head9(const WeightStore& w, float* seg) {
    pack_k64(seg, w.get("initial.0.weight"), E_HEAD_K);
    std::memcpy(seg + E_HEAD_K * 64, w.get("initial.0.bias"), 64 * sizeof(float));
    seg[E_HEAD_K * 64 + 64] = w.get("initial.1.weight")[0];
}

// One 3x3 64 -> 64 convolution into k_esr_conv's segment layout.
void pack_conv64(float* seg, const float* w, const float* bias) {
    for (int co = 0; co < 64; ++co)
        for (int ci = 0; ci < 64; ++ci)
            for (int tap = 0; tap < 9; ++tap) seg[((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * 64 + co] = w[((size_t)co * 64 + ci) * 9 + tap];
    std::memcpy(seg + E_CONV_BIAS, bias, 64 * sizeof(float));
}

// Convolution c (0, 1) of the residual block under `blk` with its BatchNorm folded; the first one carries the block's PReLU slope.
void pack_res_conv(const WeightStore& w, float* seg, const std::string& blk, int c, double eps) {
    const std::string conv = blk + std::to_string(3 * c) + ".", bn = blk + std::to_string(3 * c + 1) + ".";
    pack_conv64(seg, w.get(conv + "weight"), w.get(conv + "bias"));
    pack_bn_fold(w, bn, eps, 64, seg + E_CONV_S, seg + E_CONV_T);
    seg[E_CONV_SLOPE] = c == 0 ? w.get(blk + "2.weight")[0] : 0.f;
}

// final.*, the 9x9 tail: [ci][kh][co * 9 + kw], bias
void pack_tail9(const WeightStore& w, float* seg) {
    const float* f = w.get("final.weight");
    for (int co = 0; co < 3; ++co)
        for (int ci = 0; ci < 64; ++ci)
            for (int kh = 0; kh < 9; ++kh)
                for (int kw = 0; kw < 9; ++kw)
                    seg[((size_t)ci * 9 + kh) * E_TAIL_WROW + co * 9 + kw] = f[(((size_t)co * 64 + ci) * 9 + kh) * 9 + kw];
    std::memcpy(seg + E_TAIL_W, w.get("final.bias"), 3 * sizeof(float));
}

// The argument checks cid_esr_forward and cid_sr_forward share.
int check_image_io(const Call& cx, const void* in, int in_fmt, const void* out, int out_fmt, const void* workspace) {
    if (!in || !out || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if ((in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) || (out_fmt != CID_FMT_F32_NCHW && out_fmt != CID_FMT_U8_NHWC))
        return cx.fail(CID_ERR_INVALID, "unknown format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || (out_fmt == CID_FMT_F32_NCHW && ((uintptr_t)out & 3)))
        return cx.fail(CID_ERR_INVALID, "misaligned fp32 operand");
    return CID_OK;
}

struct EsrPlan {
    size_t x1, mid, cur, total;   // byte offsets of the three C8 tensors; `cur` ends as the tensor the tail reads
    int ctiles_x, ctiles, ttiles_x, ttiles;
};

int esr_plan(int N, int H, int W, EsrPlan& p) {
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;   // a pixel index inside one image is an int
    const size_t t = align256((size_t)N * 64 * H * W * sizeof(float));
    p.x1 = 0;
    p.mid = t;
    p.cur = 2 * t;
    p.total = 3 * t;
    p.ctiles_x = (W + D_TW - 1) / D_TW;
    p.ctiles = ((H + DiscGeom<64, 64, 1>::TH - 1) / DiscGeom<64, 64, 1>::TH) * p.ctiles_x;
    p.ttiles_x = (W + E_TAIL_TW - 1) / E_TAIL_TW;
    p.ttiles = ((H + E_TAIL_TH - 1) / E_TAIL_TH) * p.ttiles_x;
    return CID_OK;
}

}  // namespace

struct cid_esr_s : WeightStore {
    int R = 0;
    double eps[2 * kEsrMaxBlocks];
    size_t blob_floats() const { return kEsrHeadSeg + 2 * (size_t)R * kEsrConvSeg + kEsrTailSeg; }
};

namespace {
// The blob from the staged tensors: the head, the 2 R block convolutions, the tail.
void esr_pack(const cid_esr_s* h, float* b) {
    pack_head9(*h, b);
    for (int l = 0; l < 2 * h->R; ++l)
        pack_res_conv(*h, b + kEsrHeadSeg + (size_t)l * kEsrConvSeg, "residuals." + std::to_string(l / 2) + ".block.", l % 2, h->eps[l]);
    pack_tail9(*h, b + kEsrHeadSeg + 2 * (size_t)h->R * kEsrConvSeg);
}
}  // namespace

extern "C" {

int cid_esr_create(cid_esr_t* out, int num_residuals) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (num_residuals < 0 || num_residuals > kEsrMaxBlocks) return CID_ERR_INVALID;
    cid_esr_s* h = new (std::nothrow) cid_esr_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_esr", esr_keys(num_residuals));
    h->R = num_residuals;
    std::fill(h->eps, h->eps + 2 * kEsrMaxBlocks, 1e-5);
    *out = h;
    return CID_OK;
}

void cid_esr_destroy(cid_esr_t h) { delete h; }

const char* cid_esr_last_error(cid_esr_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_esr_param_key(cid_esr_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_esr_set_weight(cid_esr_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_esr_set_bn_eps(cid_esr_t h, int block, int which, double eps) {
    if (!h) return CID_ERR_INVALID;
    return h->set_bn_eps(block >= 0 && block < h->R && (which == 0 || which == 1) ? &h->eps[2 * block + which] : nullptr, eps);
}

int cid_esr_missing_weights(cid_esr_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_esr_packed_weights_bytes(cid_esr_t h) { return h ? h->blob_floats() * sizeof(float) : 0; }

int cid_esr_upload_weights(cid_esr_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, h->blob_floats(), [h](float* b) { esr_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_esr_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    EsrPlan p;
    return plan_bytes(esr_plan(N, H, W, p), p, bytes);
}

int cid_esr_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    EsrPlan p;
    const int rc = esr_plan(N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    if (s == "x1") *offset_bytes = p.x1;
    else if (s == "tail_in") *offset_bytes = p.cur;
    else return CID_ERR_KEY;
    *C = 64;
    *Hs = H;
    *Ws = W;
    *channel_block = 8;
    return CID_OK;
}

int cid_esr_forward(cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_esr_forward", stream);
    if (const int rc = check_image_io(cx, in, in_fmt, out, out_fmt, workspace)) return rc;
    EsrPlan p;
    if (esr_plan(N, H, W, p) != CID_OK) return cx.fail(CID_ERR_SHAPE, "input shape not accepted (N, H, W >= 1, H*W < 2^31)");
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_esr_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    float *x1 = reinterpret_cast<float*>(ws + p.x1), *mid = reinterpret_cast<float*>(ws + p.mid), *cur = reinterpret_cast<float*>(ws + p.cur);
    const float* blob = h->dev_blob;
    const int R = h->R;

    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        const EsrHeadArgs a{in, x1, R == 0 ? cur : nullptr, blob, H, W, n0};
        const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), (unsigned)n);
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esr_head<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_esr_head<false>, grid, dim3(D_THREADS), 0, s, a);
    })) return rc;
    for (int i = 0; i < R; ++i)
        for (int c = 0; c < 2; ++c) {
            if (const int rc = cx.launches(N, "trunk", [&](int n0, int n) {
                EsrConvArgs a{};
                a.w = blob + kEsrHeadSeg + (size_t)(2 * i + c) * kEsrConvSeg;
                a.H = H;
                a.W = W;
                a.tiles_x = p.ctiles_x;
                a.n0 = n0;
                const dim3 grid((unsigned)p.ctiles, (unsigned)n), block(D_THREADS);
                if (c == 0) {   // block.0-2: the block's input (x1 for the first block) -> mid
                    a.in = i == 0 ? x1 : cur;
                    a.out = mid;
                    hipLaunchKernelGGL(k_esr_conv<EPI_PRELU>, grid, block, 0, s, a);
                } else {        // block.3-4 and the residual sum -> cur (in place from the second block on)
                    a.in = mid;
                    a.out = cur;
                    a.res = i == 0 ? x1 : cur;
                    a.x1 = x1;
                    if (i == R - 1) hipLaunchKernelGGL(k_esr_conv<EPI_SUM>, grid, block, 0, s, a);
                    else hipLaunchKernelGGL(k_esr_conv<EPI_RES>, grid, block, 0, s, a);
                }
            })) return rc;
        }
    if (const int rc = cx.launches(N, "tail", [&](int n0, int n) {
        const EsrTailArgs a{cur, out, blob + kEsrHeadSeg + 2 * (size_t)R * kEsrConvSeg, H, W, p.ttiles_x, n0};
        const dim3 grid((unsigned)p.ttiles, (unsigned)n);
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esr_tail<true>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_esr_tail<false>, grid, dim3(E_TAIL_THREADS), 0, s, a);
    })) return rc;
    return CID_OK;
}

}  // extern "C"
