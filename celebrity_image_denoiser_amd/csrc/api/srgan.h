// The server's SRGANGenerator (cid_sr_*): weight staging, BatchNorm folding, workspace plan and launch sequence; kernels in
// srgan_kernels.h (head, upscale stage, tail) and esrgan_kernels.h (trunk); the pack helpers shared with ESRGAN: esrgan.h.  Host code.
#pragma once
#include "../srgan_kernels.h"
#include "esrgan.h"

namespace {

constexpr int kSrBlocks = 5;
constexpr size_t kSrUpSeg = (size_t)S_UP_W + 256 + 64;           // weights, bias[256] in packed order, slope (padded to 64)

KeyTable sr_keys(int stages) {
    KeyTable k;
    keys_head9(k);
    for (int i = 0; i < kSrBlocks; ++i) keys_res_block(k, "res_blocks." + std::to_string(i) + ".");
    k.conv("mid.", 64, 64, 3);
    for (int u = 0; u < stages; ++u) {
        k.conv("upscale." + std::to_string(3 * u) + ".", 256, 64, 3);
        k.tensor("upscale." + std::to_string(3 * u + 2) + ".weight", {1});
    }
    k.conv("final.", 3, 64, 9);
    return k;
}

int sr_stages(int scale) { return scale == 1 ? 0 : scale == 2 ? 1 : scale == 4 ? 2 : scale == 8 ? 3 : -1; }

struct SrPlan {
    int stages;
    size_t x0, mid, cur, up[3], total;   // byte offsets of the C8 tensors; `mid` ends as the trunk's result, up[k] is stage k's output
    int ctiles_x, ctiles;                // trunk tiles (16 x 16) of the padded image
};

int sr_plan(int N, int Hp, int Wp, int scale, SrPlan& p) {
    p.stages = sr_stages(scale);
    if (p.stages < 0) return CID_ERR_INVALID;
    if (N < 1 || Hp < 1 || Wp < 1) return CID_ERR_SHAPE;
    if ((long long)Hp * Wp > 0x7fffffffLL / ((long long)scale * scale)) return CID_ERR_SHAPE;   // a pixel index inside one image is an int
    const size_t t = align256((size_t)N * 64 * Hp * Wp * sizeof(float));
    p.x0 = 0;
    p.mid = t;
    p.cur = 2 * t;
    size_t at = 3 * t;
    for (int u = 0; u < p.stages; ++u) p.up[u] = take(at, (size_t)N * 64 * ((size_t)Hp << (u + 1)) * ((size_t)Wp << (u + 1)) * sizeof(float));
    p.total = at;
    p.ctiles_x = (Wp + D_TW - 1) / D_TW;
    p.ctiles = ((Hp + DiscGeom<64, 64, 1>::TH - 1) / DiscGeom<64, 64, 1>::TH) * p.ctiles_x;
    return CID_OK;
}

}  // namespace

struct cid_sr_s : WeightStore {
    int scale = 1, stages = 0;
    double eps[2 * kSrBlocks];
    // head, ten block convolutions, mid, the upscale stages, tail
    size_t up_off(int u) const { return kEsrHeadSeg + (2 * (size_t)kSrBlocks + 1) * kEsrConvSeg + (size_t)u * kSrUpSeg; }
    size_t tail_off() const { return up_off(stages); }
    size_t blob_floats() const { return tail_off() + kEsrTailSeg; }
};

namespace {
// Upscale stage u: [half][chunk][tap][ci % 8][128 packed columns], the columns in the order of s_up_conv_channel; bias; slope.
void sr_pack_up(const cid_sr_s* h, float* seg, int u) {
    const float* w = h->get("upscale." + std::to_string(3 * u) + ".weight");
    const float* bias = h->get("upscale." + std::to_string(3 * u) + ".bias");
    for (int J = 0; J < 256; ++J) {
        const int cc = s_up_conv_channel(J);
        for (int ci = 0; ci < 64; ++ci)
            for (int tap = 0; tap < 9; ++tap)
                seg[(size_t)(J / 128) * (64 * 9 * 128) + ((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * 128 + J % 128] = w[((size_t)cc * 64 + ci) * 9 + tap];
        seg[S_UP_BIAS + J] = bias[cc];
    }
    seg[S_UP_SLOPE] = h->get("upscale." + std::to_string(3 * u + 2) + ".weight")[0];
}

// The blob from the staged tensors: the head, the ten block convolutions, `mid` with the identity fold (s, t) = (1, 0), the upscale
// stages, the tail.
void sr_pack(const cid_sr_s* h, float* b) {
    pack_head9(*h, b);
    for (int l = 0; l < 2 * kSrBlocks; ++l)
        pack_res_conv(*h, b + kEsrHeadSeg + (size_t)l * kEsrConvSeg, "res_blocks." + std::to_string(l / 2) + ".", l % 2, h->eps[l]);
    float* mid = b + kEsrHeadSeg + 2 * (size_t)kSrBlocks * kEsrConvSeg;   // bias only; fmaf(1, z, 0) = z
    pack_conv64(mid, h->get("mid.weight"), h->get("mid.bias"));
    std::fill(mid + E_CONV_S, mid + E_CONV_S + 64, 1.f);
    for (int u = 0; u < h->stages; ++u) sr_pack_up(h, b + h->up_off(u), u);
    pack_tail9(*h, b + h->tail_off());
}
}  // namespace

extern "C" {

int cid_sr_create(cid_sr_t* out, int scale_factor) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (sr_stages(scale_factor) < 0) return CID_ERR_INVALID;
    cid_sr_s* h = new (std::nothrow) cid_sr_s();
    if (!h) return CID_ERR_INVALID;
    h->scale = scale_factor;
    h->stages = sr_stages(scale_factor);
    h->init("cid_sr", sr_keys(h->stages));
    std::fill(h->eps, h->eps + 2 * kSrBlocks, 1e-5);
    *out = h;
    return CID_OK;
}

void cid_sr_destroy(cid_sr_t h) { delete h; }

const char* cid_sr_last_error(cid_sr_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_sr_param_key(cid_sr_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_sr_set_weight(cid_sr_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_sr_set_bn_eps(cid_sr_t h, int block, int which, double eps) {
    if (!h) return CID_ERR_INVALID;
    return h->set_bn_eps(block >= 0 && block < kSrBlocks && (which == 0 || which == 1) ? &h->eps[2 * block + which] : nullptr, eps);
}

int cid_sr_missing_weights(cid_sr_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_sr_packed_weights_bytes(cid_sr_t h) { return h ? h->blob_floats() * sizeof(float) : 0; }

int cid_sr_upload_weights(cid_sr_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, h->blob_floats(), [h](float* b) { sr_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_sr_workspace_bytes(int N, int Hp, int Wp, int scale_factor, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    SrPlan p;
    return plan_bytes(sr_plan(N, Hp, Wp, scale_factor, p), p, bytes);
}

int cid_sr_stage_view(const char* stage, int N, int Hp, int Wp, int scale_factor, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                      int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    SrPlan p;
    const int rc = sr_plan(N, Hp, Wp, scale_factor, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    int shift = 0;
    if (s == "x0") *offset_bytes = p.x0;
    else if (s == "trunk") *offset_bytes = p.mid;
    else if (s == "up1" && p.stages >= 2) *offset_bytes = p.up[0], shift = 1;
    else if (s == "up2" && p.stages >= 3) *offset_bytes = p.up[1], shift = 2;
    else if (s == "tail_in") *offset_bytes = p.stages ? p.up[p.stages - 1] : p.mid, shift = p.stages;
    else return CID_ERR_KEY;
    *C = 64;
    *Hs = Hp << shift;
    *Ws = Wp << shift;
    *channel_block = 8;
    return CID_OK;
}

int cid_sr_forward(cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, int pad_left, int pad_top,
                   int pad_right, int pad_bottom, unsigned flags, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_sr_forward", stream);
    if (const int rc = check_image_io(cx, in, in_fmt, out, out_fmt, workspace)) return rc;
    if (flags & ~(unsigned)CID_SR_RAW) return cx.fail(CID_ERR_INVALID, "unknown flags");
    if ((flags & CID_SR_RAW) && out_fmt != CID_FMT_F32_NCHW) return cx.fail(CID_ERR_INVALID, "CID_SR_RAW needs an fp32 output");
    for (const int pad : {pad_left, pad_top, pad_right, pad_bottom})
        if (pad < 0 || pad > 4096) return cx.fail(CID_ERR_INVALID, "pads must lie in [0, 4096]");
    if (N < 1 || H < 1 || W < 1 || H > 0x7fffffff - 8192 || W > 0x7fffffff - 8192)
        return cx.fail(CID_ERR_SHAPE, "input shape not accepted (N, H, W >= 1)");
    const int Hp = H + pad_top + pad_bottom, Wp = W + pad_left + pad_right;
    SrPlan p;
    if (sr_plan(N, Hp, Wp, h->scale, p) != CID_OK)
        return cx.fail(CID_ERR_SHAPE, "input shape not accepted (scale^2 * Hp * Wp < 2^31)");
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_sr_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    float *x0 = reinterpret_cast<float*>(ws + p.x0), *mid = reinterpret_cast<float*>(ws + p.mid), *cur = reinterpret_cast<float*>(ws + p.cur);
    const float* blob = h->dev_blob;

    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        const SrHeadArgs a{in, x0, blob, H, W, Hp, Wp, pad_left, pad_top, n0};
        const dim3 grid((unsigned)(((long long)Hp * Wp + D_THREADS - 1) / D_THREADS), (unsigned)n);
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_sr_head<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_sr_head<false>, grid, dim3(D_THREADS), 0, s, a);
    })) return rc;
    // launches 0 .. 9: the blocks' convolutions (x0 or cur -> mid -> cur); launch 10: mid(cur) + x0 -> mid
    for (int l = 0; l <= 2 * kSrBlocks; ++l) {
        if (const int rc = cx.launches(N, "trunk", [&](int n0, int n) {
            EsrConvArgs a{};
            a.w = blob + kEsrHeadSeg + (size_t)l * kEsrConvSeg;
            a.H = Hp;
            a.W = Wp;
            a.tiles_x = p.ctiles_x;
            a.n0 = n0;
            const dim3 grid((unsigned)p.ctiles, (unsigned)n), block(D_THREADS);
            if (l == 2 * kSrBlocks) {
                a.in = cur;
                a.out = mid;
                a.res = x0;
                hipLaunchKernelGGL(k_esr_conv<EPI_RES>, grid, block, 0, s, a);
            } else if (l % 2 == 0) {
                a.in = l == 0 ? x0 : cur;
                a.out = mid;
                hipLaunchKernelGGL(k_esr_conv<EPI_PRELU>, grid, block, 0, s, a);
            } else {
                a.in = mid;
                a.out = cur;
                hipLaunchKernelGGL(k_esr_conv<EPI_BN>, grid, block, 0, s, a);
            }
        })) return rc;
    }
    const float* u = mid;
    int Hu = Hp, Wu = Wp;
    for (int k = 0; k < p.stages; ++k) {
        float* dst = reinterpret_cast<float*>(ws + p.up[k]);
        const int tiles_x = (Wu + D_TW - 1) / D_TW;
        const int tiles = ((Hu + DiscGeom<64, 128, 1>::TH - 1) / DiscGeom<64, 128, 1>::TH) * tiles_x;
        if (const int rc = cx.launches(N, "upscale", [&](int n0, int n) {
            const SrUpArgs a{u, dst, blob + h->up_off(k), Hu, Wu, tiles_x, n0};
            hipLaunchKernelGGL(k_sr_up<>, dim3((unsigned)tiles, (unsigned)n, 2), dim3(D_THREADS), 0, s, a);
        })) return rc;
        u = dst;
        Hu *= 2;
        Wu *= 2;
    }
    const int ttiles_x = (Wu + E_TAIL_TW - 1) / E_TAIL_TW;
    const int ttiles = ((Hu + E_TAIL_TH - 1) / E_TAIL_TH) * ttiles_x;
    if (const int rc = cx.launches(N, "tail", [&](int n0, int n) {
        const EsrTailArgs a{u, out, blob + h->tail_off(), Hu, Wu, ttiles_x, n0};
        const dim3 grid((unsigned)ttiles, (unsigned)n);
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_sr_tail<SR_OUT_U8>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else if (flags & CID_SR_RAW) hipLaunchKernelGGL(k_sr_tail<SR_OUT_RAW>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_sr_tail<SR_OUT_F32>, grid, dim3(E_TAIL_THREADS), 0, s, a);
    })) return rc;
    return CID_OK;
}

}  // extern "C"
