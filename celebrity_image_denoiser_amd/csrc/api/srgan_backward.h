// The SRGAN generator's backward pass in train mode (cid_sr_saved_bytes, cid_sr_forward_saved, cid_sr_backward, cid_sr_saved_masks):
// saved-buffer and workspace plans, argument checks and the launch sequence.  The saved forward is cid_sr_forward_train's run
// (sr_train_run, srgan_train.h) pointed into the saved buffer; the backward's kernels are in srgan_bwd_kernels.h, with
// k_disc_wgrad_reduce and k_disc_masks of disc_bwd_kernels.h.  Host code.
#pragma once
#include "../srgan_bwd_kernels.h"
#include "srgan_train.h"

namespace {

// What cid_sr_forward_saved keeps for one call.
struct SrSavedPlan {
    int stages;
    size_t v0, z[S_TRAIN_BNS], t, v[3], st, mi, out, total;
};

int sr_saved_plan(int N, int H, int W, int scale, SrSavedPlan& q) {
    SrTrainPlan p;
    if (const int rc = sr_train_plan(N, H, W, scale, p)) return rc;
    q.stages = p.stages;
    const size_t t = (size_t)N * 64 * H * W * sizeof(float);
    size_t at = 0;
    q.v0 = take(at, t);
    for (int l = 0; l < S_TRAIN_BNS; ++l) q.z[l] = take(at, t);
    q.t = take(at, t);
    for (int k = 0; k < q.stages; ++k) q.v[k] = take(at, t << (2 * (k + 1)));
    q.st = take(at, (size_t)S_TRAIN_BNS * 128 * sizeof(float));
    q.mi = take(at, (size_t)S_TRAIN_BNS * 128 * sizeof(double));
    q.out = take(at, ((size_t)N * 3 * H * W * sizeof(float)) << (2 * q.stages));
    q.total = at;
    return CID_OK;
}

struct SrSavedBufs {
    float* v0;
    float* z[S_TRAIN_BNS];
    float* t;
    float* v[3];
    float* st;
    double* mi;
    float* out;
};

SrSavedBufs sr_saved_bufs(void* saved, const SrSavedPlan& q) {
    char* sv = static_cast<char*>(saved);
    SrSavedBufs b{};
    b.v0 = reinterpret_cast<float*>(sv + q.v0);
    for (int l = 0; l < S_TRAIN_BNS; ++l) b.z[l] = reinterpret_cast<float*>(sv + q.z[l]);
    b.t = reinterpret_cast<float*>(sv + q.t);
    for (int k = 0; k < q.stages; ++k) b.v[k] = reinterpret_cast<float*>(sv + q.v[k]);
    b.st = reinterpret_cast<float*>(sv + q.st);
    b.mi = reinterpret_cast<double*>(sv + q.mi);
    b.out = reinterpret_cast<float*>(sv + q.out);
    return b;
}

// Workspace of one backward call.  A and B hold the gradients of the tail's input and of the stages' inputs in turn (A at the output's
// size, B at half of it), T1 and T2 the trunk's.
constexpr int kSrWgSplits = 128, kSrWgUpSplits = 32, kSrW9Splits = 256, kSrTwSplits = 512;   // workgroups of the weight gradients

struct SrBwdPlan {
    int stages;
    size_t A, B, T1, T2, coef, bnslab, chan, part, part_b, part9, total;
};

int sr_bwd_plan(int N, int H, int W, int scale, SrBwdPlan& q) {
    SrTrainPlan p;
    if (const int rc = sr_train_plan(N, H, W, scale, p)) return rc;
    q.stages = p.stages;
    const size_t n = (size_t)N, t = n * 64 * H * W * sizeof(float);
    const size_t strips = (((size_t)H * W << (2 * q.stages)) + D_BN_STRIP - 1) / D_BN_STRIP;
    size_t at = 0;
    q.A = take(at, t << (2 * q.stages));
    q.B = take(at, q.stages ? t << (2 * (q.stages - 1)) : 0);
    q.T1 = take(at, t);
    q.T2 = take(at, t);
    q.coef = take(at, (size_t)64 * D_COEF * sizeof(float));
    q.bnslab = take(at, (size_t)64 * 3 * n * strips * sizeof(double));
    q.chan = take(at, 64 * sizeof(double));
    q.part = take(at, std::max((size_t)kSrWgSplits * 4 * 64, (size_t)kSrWgUpSplits * 4 * 256) * 144 * sizeof(float));
    q.part_b = take(at, std::max((size_t)kSrWgSplits * 64, (size_t)kSrWgUpSplits * 256) * sizeof(double));
    q.part9 = take(at, (size_t)std::max(kSrW9Splits, kSrTwSplits) * 64 * SG_W9_K * sizeof(double));
    q.total = at;
    return CID_OK;
}

// The kernel + reduce pairs cid_sr_backward and cid_esr_backward (esrgan_backward.h) launch, over one call's stream and scratch regions.
struct SrgLaunch {
    const Call& cx;
    int N;
    float* coef;
    double* bnslab;
    double* chan;
    float* part;
    double* part_b;
    double* part9;

    // sums of one tensor with a PReLU: strips -> per channel -> the slope's gradient
    template <class K>
    int slope_sums(K kernel, const SrgDz& dz, const float* st, const double* mi, const float* slope, const float* gamma, float* dgamma,
                   float* dbeta, float* dslope, int Hl, int Wl, const char* what) const {
        const hipStream_t s = cx.s;
        const dim3 block(D_THREADS);
        const long long P = (long long)Hl * Wl;
        const int strips = (int)((P + D_BN_STRIP - 1) / D_BN_STRIP);
        const long long rows = (long long)N * strips;
        if (const int rc = cx.launches(N, what, [&](int n0, int n) {
            const SrgBnPartArgs a{dz, st, mi, slope, bnslab, rows, P, strips, n0};
            hipLaunchKernelGGL(kernel, dim3((unsigned)strips, (unsigned)n), block, 0, s, a);
        })) return rc;
        const SrgBnRedArgs r{bnslab, rows, (double)N * (double)P, gamma, st, mi, slope, coef, dgamma, dbeta, chan};
        hipLaunchKernelGGL(k_srg_bn_reduce, dim3(64), block, 0, s, r);
        if (slope && dslope) hipLaunchKernelGGL(k_srg_sum, dim3(1), block, 0, s, chan, 64LL, dslope);
        return hipPeekAtLastError() == hipSuccess ? CID_OK : cx.hip(what);
    }
    // weight and bias gradient of a 3x3 convolution at Hl x Wl (parts = 4: an upscale stage's 256 packed columns)
    template <class K>
    int wgrad(K kernel, int parts, const SrgDz& dz, const float* ain, const float* st_in, const float* slope_in, float* dw, float* db, int Hl,
              int Wl, const char* what) const {
        if (!dw && !db) return CID_OK;
        const hipStream_t s = cx.s;
        const dim3 block(D_THREADS);
        const int tiles_x = (Wl + D_TW - 1) / D_TW, tiles = ((Hl + D_WG_TH - 1) / D_WG_TH) * tiles_x;
        const long long items = (long long)N * tiles;
        const int splits = (int)std::min<long long>(items, parts == 1 ? kSrWgSplits : kSrWgUpSplits);
        const SrgWgradArgs a{dz, ain, st_in, slope_in, part, part_b, items, splits, Hl, Wl, tiles_x, tiles};
        hipLaunchKernelGGL(kernel, dim3((unsigned)splits, 4, (unsigned)parts), block, 0, s, a);
        if (parts == 1) {
            const DiscWgradReduceArgs r{part, part_b, dw, db, splits, 64, 64};
            hipLaunchKernelGGL(k_disc_wgrad_reduce, dim3((64 * 64 * 9 + 64 + D_THREADS - 1) / D_THREADS), block, 0, s, r);
        } else {
            const SrgWgradReduceArgs r{part, part_b, dw, db, splits};
            hipLaunchKernelGGL(k_srg_wgrad_reduce, dim3((256 * 64 * 9 + 256 + D_THREADS - 1) / D_THREADS), block, 0, s, r);
        }
        return hipPeekAtLastError() == hipSuccess ? CID_OK : cx.hip(what);
    }
    // data gradient of a 3x3 convolution: out = add + dgrad (add null: dgrad)
    template <class K>
    int dgrad(K kernel, const SrgDz& dz, const float* w, float* out, const float* add, int Hl, int Wl, const char* what) const {
        const hipStream_t s = cx.s;
        const int tiles_x = (Wl + D_TW - 1) / D_TW, tiles = ((Hl + 15) / 16) * tiles_x;
        return cx.launches(N, what, [&](int n0, int n) {
            const SrgDgradArgs a{dz, w, out, add, Hl, Wl, tiles_x, n0};
            hipLaunchKernelGGL(kernel, dim3((unsigned)tiles, (unsigned)n), dim3(D_THREADS), 0, s, a);
        });
    }
    // the reduce of k_srg_wgrad243's and k_srg_tail_wgrad's partials
    int reduce9(float* dw, float* db, int splits, int head, const char* what) const {
        const SrgWgrad9ReduceArgs r{part9, dw, db, splits, head};
        hipLaunchKernelGGL(k_srg_wgrad243_reduce, dim3((64 * SG_W9_K + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, cx.s, r);
        return hipPeekAtLastError() == hipSuccess ? CID_OK : cx.hip(what);
    }
};

}  // namespace

extern "C" {

int cid_sr_saved_bytes(int N, int H, int W, int scale_factor, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    SrSavedPlan q;
    return plan_bytes(sr_saved_plan(N, H, W, scale_factor, q), q, bytes);
}

int cid_sr_forward_saved(cid_sr_t h, const void* in, int in_fmt, float* out, int N, int H, int W, unsigned flags, const cid_disc_bn* bn,
                         void* saved, size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_sr_forward_saved", stream);
    if (!saved) return cx.fail(CID_ERR_INVALID, "null pointer");
    SrTrainPlan p;
    if (const int rc = sr_train_check(cx, h, in, in_fmt, out, CID_FMT_F32_NCHW, N, H, W, flags, bn, workspace, p)) return rc;
    SrSavedPlan q;
    sr_saved_plan(N, H, W, h->scale, q);
    if (const int rc = cx.room(saved, saved_bytes, q.total, "cid_sr_saved_bytes", "saved buffer")) return rc;
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_sr_train_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    const SrSavedBufs sv = sr_saved_bufs(saved, q);
    SrTrainBufs b = sr_train_bufs(workspace, p);
    for (int l = 0; l < S_TRAIN_BNS; ++l) b.z[l] = sv.z[l];
    b.trunk = sv.t;
    b.st = sv.st;
    b.mi = sv.mi;
    b.pre0 = sv.v0;
    for (int k = 0; k < p.stages; ++k) b.pre_up[k] = sv.v[k];
    if (const int rc = sr_train_run(cx, h, in, in_fmt, out, CID_FMT_F32_NCHW, N, H, W, flags, bn, p, b)) return rc;
    if (!(flags & CID_SR_RAW) &&   // tanh's derivative reads the result
        hipMemcpyAsync(sv.out, out, ((size_t)N * 3 * H * W * sizeof(float)) << (2 * p.stages), hipMemcpyDeviceToDevice, cx.s) != hipSuccess)
        return cx.hip("copy of out");
    return CID_OK;
}

int cid_sr_backward_workspace_bytes(int N, int H, int W, int scale_factor, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    SrBwdPlan q;
    return plan_bytes(sr_bwd_plan(N, H, W, scale_factor, q), q, bytes);
}

int cid_sr_backward(cid_sr_t h, const void* in, int in_fmt, const float* grad_out, int N, int H, int W, unsigned flags,
                    const cid_disc_bn* bn, const void* saved, size_t saved_bytes, const cid_sr_grads* g, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_sr_backward", stream);
    if (!in || !grad_out || !bn || !saved || !g || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (!fmt_ok(in, in_fmt)) return cx.fail(CID_ERR_INVALID, "unknown format or misaligned fp32 operand");
    if ((uintptr_t)grad_out & 3) return cx.fail(CID_ERR_INVALID, "misaligned grad_out");
    if (flags & ~(unsigned)CID_SR_RAW) return cx.fail(CID_ERR_INVALID, "unknown flags");
    for (int l = 0; l < S_TRAIN_BNS; ++l)
        if (!bn[l].gamma) return cx.fail(CID_ERR_INVALID, "null BatchNorm pointer");
    static_assert(sizeof(cid_sr_grads) % sizeof(float*) == 0, "pointers only");
    for (size_t i = 0; i < sizeof(cid_sr_grads) / sizeof(float*); ++i)
        if ((uintptr_t)reinterpret_cast<float* const*>(g)[i] & 3) return cx.fail(CID_ERR_INVALID, "misaligned gradient tensor");
    SrSavedPlan sp;
    if (sr_saved_plan(N, H, W, h->scale, sp) != CID_OK) return sr_train_shape_fail(cx, N, H, W);
    if (const int rc = cx.room(saved, saved_bytes, sp.total, "cid_sr_saved_bytes", "saved buffer")) return rc;
    SrBwdPlan q;
    sr_bwd_plan(N, H, W, h->scale, q);
    if (const int rc = cx.room(workspace, workspace_bytes, q.total, "cid_sr_backward_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;

    const hipStream_t s = cx.s;
    const SrSavedBufs sv = sr_saved_bufs(const_cast<void*>(saved), sp);
    char* ws = static_cast<char*>(workspace);
    float* AB[2] = {reinterpret_cast<float*>(ws + q.A), reinterpret_cast<float*>(ws + q.B)};
    float* T[2] = {reinterpret_cast<float*>(ws + q.T1), reinterpret_cast<float*>(ws + q.T2)};
    float* coef = reinterpret_cast<float*>(ws + q.coef);
    double* bnslab = reinterpret_cast<double*>(ws + q.bnslab);
    double* chan = reinterpret_cast<double*>(ws + q.chan);
    float* part = reinterpret_cast<float*>(ws + q.part);
    double* part_b = reinterpret_cast<double*>(ws + q.part_b);
    double* part9 = reinterpret_cast<double*>(ws + q.part9);
    const float* blob = h->dev_blob;
    const int S = q.stages, raw = (flags & CID_SR_RAW) ? 1 : 0;
    const int Hs = H << S, Ws = W << S;
    const float* head_slope = blob + E_HEAD_K * 64 + 64;
    const auto conv_seg = [&](int l) { return blob + kEsrHeadSeg + (size_t)l * kEsrConvSeg; };
    const auto block_slope = [&](int i) { return conv_seg(2 * i) + E_CONV_SLOPE; };
    const auto up_slope = [&](int k) { return blob + h->up_off(k) + S_UP_SLOPE; };
    const dim3 block(D_THREADS);

    const SrgLaunch lx{cx, N, coef, bnslab, chan, part, part_b, part9};
    // ---- final: bias, weights, and the gradient of its input -> A
    if (g->final_b) {
        const long long P = (long long)Hs * Ws;
        const int strips = (int)((P + D_BN_STRIP - 1) / D_BN_STRIP);
        const long long rows = (long long)N * strips;
        if (const int rc = cx.launches(N, "final bias", [&](int n0, int n) {
            const SrgTailBiasArgs a{grad_out, sv.out, bnslab, rows, P, strips, raw, n0};
            hipLaunchKernelGGL(k_srg_tail_bias_part, dim3((unsigned)strips, (unsigned)n), block, 0, s, a);
        })) return rc;
        hipLaunchKernelGGL(k_srg_sum, dim3(3), block, 0, s, bnslab, rows, g->final_b);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("final bias");
    }
    if (g->final_w) {
        const int tiles_x = (Ws + D_TW - 1) / D_TW, tiles = ((Hs + D_WG_TH - 1) / D_WG_TH) * tiles_x;
        const long long items = (long long)N * tiles;
        const int splits = (int)std::min<long long>(items, kSrTwSplits);
        const SrgTailWgradArgs a{S ? sv.v[S - 1] : sv.t, S ? up_slope(S - 1) : nullptr, grad_out, sv.out, part9, items, splits, Hs, Ws,
                                 tiles_x, tiles, raw};
        if (S) hipLaunchKernelGGL(k_srg_tail_wgrad<true>, dim3((unsigned)splits), block, 0, s, a);
        else hipLaunchKernelGGL(k_srg_tail_wgrad<false>, dim3((unsigned)splits), block, 0, s, a);
        if (const int rc = lx.reduce9(g->final_w, nullptr, splits, 0, "final wgrad")) return rc;
    }
    {
        const int tiles_x = (Ws + D_TW - 1) / D_TW, tiles = ((Hs + 15) / 16) * tiles_x;
        if (const int rc = cx.launches(N, "final dgrad", [&](int n0, int n) {
            const SrgTailDgradArgs a{grad_out, sv.out, blob + h->tail_off(), AB[0], Hs, Ws, tiles_x, raw, n0};
            hipLaunchKernelGGL(k_srg_tail_dgrad, dim3((unsigned)tiles, (unsigned)n), block, 0, s, a);
        })) return rc;
    }
    // ---- the upscale stages, last first: A -> B -> A ...; `cur` ends as the gradient of t
    int cur = 0;
    for (int k = S - 1; k >= 0; --k) {
        const int Hk = H << k, Wk = W << k;
        const SrgDz dz{sv.v[k], AB[cur], up_slope(k)};
        if (g->up_slope[k])
            if (const int rc = lx.slope_sums(k_srg_bn_part<SG_DZ_PRELU>, dz, nullptr, nullptr, up_slope(k), nullptr, nullptr, nullptr,
                                          g->up_slope[k], 2 * Hk, 2 * Wk, "upscale slope"))
                return rc;
        const int rc = k == 0 ? lx.wgrad(k_srg_wgrad<SG_DZ_SHUFFLE, SG_IN_RAW, 256>, 4, dz, sv.t, nullptr, nullptr, g->up_w[k], g->up_b[k], Hk, Wk,
                                      "upscale wgrad")
                              : lx.wgrad(k_srg_wgrad<SG_DZ_SHUFFLE, SG_IN_PRELU, 256>, 4, dz, sv.v[k - 1], nullptr, up_slope(k - 1), g->up_w[k],
                                      g->up_b[k], Hk, Wk, "upscale wgrad");
        if (rc) return rc;
        if (const int rc2 = lx.dgrad(k_srg_dgrad<256, SG_DZ_SHUFFLE>, dz, blob + h->up_off(k), AB[1 - cur], nullptr, Hk, Wk, "upscale dgrad"))
            return rc2;
        cur = 1 - cur;
    }
    const float* dt = AB[cur];
    // ---- mid
    {
        const SrgDz dz{nullptr, dt, nullptr};
        if (const int rc = lx.wgrad(k_srg_wgrad<SG_DZ_PLAIN, SG_IN_BN>, 1, dz, sv.z[9], sv.st + 9 * 128, nullptr, g->mid_w, g->mid_b, H, W, "mid wgrad"))
            return rc;
        if (const int rc = lx.dgrad(k_srg_dgrad<64, SG_DZ_PLAIN>, dz, conv_seg(S_TRAIN_BNS), T[0], nullptr, H, W, "mid dgrad")) return rc;
    }
    // ---- BatchNorm l and convolution l, l = 9 .. 0: T[tc] holds the gradient of A_l(BN_l(z_l))
    int tc = 0;
    for (int l = S_TRAIN_BNS - 1; l >= 0; --l) {
        const float* act = l % 2 == 0 ? block_slope(l / 2) : nullptr;   // the PReLU behind BN_l
        const SrgDz dz{sv.z[l], T[tc], coef};
        if (const int rc = lx.slope_sums(k_srg_bn_part<SG_DZ_BN>, dz, sv.st + l * 128, sv.mi + l * 128, act, bn[l].gamma, g->gamma[l], g->beta[l],
                                      act ? g->slope[l / 2] : nullptr, H, W, "bn sums"))
            return rc;
        int rc;
        if (l == 0)
            rc = lx.wgrad(k_srg_wgrad<SG_DZ_BN, SG_IN_PRELU>, 1, dz, sv.v0, nullptr, head_slope, g->conv_w[l], g->conv_b[l], H, W, "wgrad");
        else if (l % 2)
            rc = lx.wgrad(k_srg_wgrad<SG_DZ_BN, SG_IN_BN_PRELU>, 1, dz, sv.z[l - 1], sv.st + (l - 1) * 128, block_slope((l - 1) / 2), g->conv_w[l],
                       g->conv_b[l], H, W, "wgrad");
        else
            rc = lx.wgrad(k_srg_wgrad<SG_DZ_BN, SG_IN_BN>, 1, dz, sv.z[l - 1], sv.st + (l - 1) * 128, nullptr, g->conv_w[l], g->conv_b[l], H, W, "wgrad");
        if (rc) return rc;
        // x0 has two gradients: through res_blocks.0.0 and through the skip into t
        if (const int rc2 = lx.dgrad(k_srg_dgrad<64, SG_DZ_BN>, dz, conv_seg(l), T[1 - tc], l == 0 ? dt : nullptr, H, W, "dgrad")) return rc2;
        tc = 1 - tc;
    }
    // ---- head: T[tc] holds the gradient of x0
    const SrgDz dz0{sv.v0, T[tc], head_slope};
    if (g->head_slope)
        if (const int rc = lx.slope_sums(k_srg_bn_part<SG_DZ_PRELU>, dz0, nullptr, nullptr, head_slope, nullptr, nullptr, nullptr, g->head_slope, H,
                                      W, "head slope"))
            return rc;
    if (!g->head_w && !g->head_b) return CID_OK;
    const int segs = (W + SG_W9_PX - 1) / SG_W9_PX;
    const long long items = (long long)N * H * segs;
    const int splits = (int)std::min<long long>(items, kSrW9Splits);
    const SrgWgrad9Args a9{dz0, in, part9, items, splits, segs, H, W, in_fmt == CID_FMT_U8_NHWC};
    hipLaunchKernelGGL(k_srg_wgrad243<>, dim3((unsigned)splits), block, 0, s, a9);
    return lx.reduce9(g->head_w, g->head_b, splits, 1, "head wgrad");
}

int cid_sr_pack_weights_device(cid_sr_t h, const float* const* dev_params, const cid_disc_bn* bn, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!dev_params || !bn || !device_blob) return h->fail(CID_ERR_INVALID, "cid_sr_pack_weights_device: null pointer");
    const int count = 3 + 9 * kSrBlocks + 2 + 3 * h->stages + 2;
    for (int i = 0; i < count; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3))
            return h->fail(CID_ERR_INVALID, "cid_sr_pack_weights_device: null or misaligned parameter pointer");
    for (int l = 0; l < S_TRAIN_BNS; ++l) {
        if (!bn[l].gamma || !bn[l].beta || !bn[l].running_mean || !bn[l].running_var)
            return h->fail(CID_ERR_INVALID, "cid_sr_pack_weights_device: null BatchNorm pointer");
        if (!disc_finite_nonneg(bn[l].eps)) return h->fail(CID_ERR_INVALID, "cid_sr_pack_weights_device: eps must be finite and >= 0");
    }
    if ((uintptr_t)device_blob & 255) return h->fail(CID_ERR_WORKSPACE, "cid_sr_pack_weights_device: blob must be 256-byte aligned");
    static_assert(SG_PACK_HEAD == (int)kEsrHeadSeg && SG_PACK_CONV == (int)kEsrConvSeg && SG_PACK_UP == (int)kSrUpSeg &&
                      SG_PACK_TAIL == (int)kEsrTailSeg, "the segments of sr_pack");
    // dev_params in the module's parameter order: initial.0.{weight,bias}, initial.1.weight, per block 0.{w,b} 1.{w,b} 2.w 3.{w,b}
    // 4.{w,b}, mid.{w,b}, per stage 3k.{w,b} (3k+2).w, final.{w,b}
    SrgPackArgs a{};
    const float* const* p = dev_params;
    a.head_w = p[0], a.head_b = p[1], a.head_slope = p[2];
    p += 3;
    for (int i = 0; i < kSrBlocks; ++i, p += 9) {
        a.conv_w[2 * i] = p[0], a.conv_b[2 * i] = p[1];
        a.slope[i] = p[4];
        a.conv_w[2 * i + 1] = p[5], a.conv_b[2 * i + 1] = p[6];
    }
    a.conv_w[S_TRAIN_BNS] = p[0], a.conv_b[S_TRAIN_BNS] = p[1];
    p += 2;
    for (int u = 0; u < h->stages; ++u, p += 3) a.up_w[u] = p[0], a.up_b[u] = p[1], a.up_slope[u] = p[2];
    a.tail_w = p[0], a.tail_b = p[1];
    for (int l = 0; l < S_TRAIN_BNS; ++l) {
        a.gamma[l] = static_cast<const float*>(bn[l].gamma), a.beta[l] = static_cast<const float*>(bn[l].beta);
        a.mean[l] = static_cast<const float*>(bn[l].running_mean), a.var[l] = static_cast<const float*>(bn[l].running_var);
        a.eps[l] = bn[l].eps;
    }
    a.blob = static_cast<float*>(device_blob);
    a.stages = h->stages;
    const int longest = std::max({SG_PACK_HEAD, SG_PACK_CONV, SG_PACK_UP, SG_PACK_TAIL});
    hipLaunchKernelGGL(k_srg_pack, dim3((longest + D_THREADS - 1) / D_THREADS, S_TRAIN_BNS + 3 + h->stages), dim3(D_THREADS), 0,
                       static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return h->fail(CID_ERR_HIP, "cid_sr_pack_weights_device: launch failed");
    h->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_sr_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int scale_factor, unsigned char* const* masks,
                       void* stream) {
    if (!saved || !masks) return CID_ERR_INVALID;
    SrSavedPlan sp;
    if (const int rc = sr_saved_plan(N, H, W, scale_factor, sp)) return rc;
    for (int i = 0; i < 6 + sp.stages; ++i)
        if (!masks[i]) return CID_ERR_INVALID;
    if (saved_bytes < sp.total || ((uintptr_t)saved & 255)) return CID_ERR_WORKSPACE;
    const SrSavedBufs sv = sr_saved_bufs(const_cast<void*>(saved), sp);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = 0; i < 6 + sp.stages; ++i) {
        const int k = i - 6;   // the stage, for i >= 6
        const long long P = i < 6 ? (long long)H * W : ((long long)H * W) << (2 * (k + 1));
        const float* z = i == 0 ? sv.v0 : (i < 6 ? sv.z[2 * (i - 1)] : sv.v[k]);
        const float* st = i >= 1 && i < 6 ? sv.st + 2 * (i - 1) * 128 : nullptr;
        const DiscMaskArgs a{z, st, masks[i], (long long)N * 64 * P, P, 64};
        const long long blocks = (a.total + D_THREADS - 1) / D_THREADS;
        if (blocks > 0x7fffffffLL) return CID_ERR_SHAPE;
        hipLaunchKernelGGL(k_disc_masks, dim3((unsigned)blocks), dim3(D_THREADS), 0, s, a);
        if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
    }
    return CID_OK;
}

}  // extern "C"
