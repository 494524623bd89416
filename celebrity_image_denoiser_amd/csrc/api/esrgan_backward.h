// The ESRGAN generator's backward pass in train mode (cid_esr_saved_bytes, cid_esr_forward_saved, cid_esr_backward_workspace_bytes,
// cid_esr_backward, cid_esr_pack_weights_device, cid_esr_saved_masks): saved-buffer and workspace plans, argument checks and the launch
// sequence.  The saved forward is cid_esr_forward_train's run (esr_train_run, esrgan_train.h) pointed into the saved buffer; the
// backward's kernels are srgan_bwd_kernels.h's, with k_esrg_join and k_esrg_pack of esrgan_bwd_kernels.h and k_disc_wgrad_reduce and
// k_disc_masks of disc_bwd_kernels.h.  The launches go through cid_sr_backward's SrgLaunch (srgan_backward.h), whose workgroup caps of the weight gradients are this call's too.  Host code.
#pragma once
#include "../esrgan_bwd_kernels.h"
#include "esrgan_train.h"
#include "srgan_backward.h"

namespace {

// What cid_esr_forward_saved keeps for one call: 3 R + 1 tensors for R >= 1 (v0, the 2 R raw z, r_0 .. r_{R-2}, tail_in), v0 and
// tail_in for R = 0, and the BatchNorm tables.
struct EsrSavedPlan {
    size_t v0, z[2 * kEsrMaxBlocks], r[kEsrMaxBlocks], tail_in, st, mi, total;
};

int esr_saved_plan(int N, int H, int W, int R, EsrSavedPlan& q) {
    EsrTrainPlan p;
    if (const int rc = esr_train_plan(N, H, W, R, p)) return rc;
    const size_t t = (size_t)N * 64 * H * W * sizeof(float);
    size_t at = 0;
    q.v0 = take(at, t);
    for (int l = 0; l < 2 * R; ++l) q.z[l] = take(at, t);
    for (int i = 0; i + 1 < R; ++i) q.r[i] = take(at, t);
    q.tail_in = take(at, t);
    q.st = take(at, (size_t)2 * R * 128 * sizeof(float));
    q.mi = take(at, (size_t)2 * R * 128 * sizeof(double));
    q.total = at;
    return CID_OK;
}

struct EsrSavedBufs {
    float* v0;
    float* z[2 * kEsrMaxBlocks];
    float* r[kEsrMaxBlocks];
    float* tail_in;
    float* st;     // BatchNorm l's (scale, shift) at st + 128 l
    double* mi;    // BatchNorm l's (mean, invstd) at mi + 128 l
};

EsrSavedBufs esr_saved_bufs(void* saved, int R, const EsrSavedPlan& q) {
    char* sv = static_cast<char*>(saved);
    EsrSavedBufs b{};
    b.v0 = reinterpret_cast<float*>(sv + q.v0);
    for (int l = 0; l < 2 * R; ++l) b.z[l] = reinterpret_cast<float*>(sv + q.z[l]);
    for (int i = 0; i + 1 < R; ++i) b.r[i] = reinterpret_cast<float*>(sv + q.r[i]);
    b.tail_in = reinterpret_cast<float*>(sv + q.tail_in);
    b.st = reinterpret_cast<float*>(sv + q.st);
    b.mi = reinterpret_cast<double*>(sv + q.mi);
    return b;
}

// Workspace of one backward call.  A holds dT, the gradient of tail_in, to the end (the outer skip hands it to x1); T the gradient of
// a block's PReLU output and at last the gradient of x1; G1 and G2 the gradients G_i of the block outputs in turn (R >= 1).
struct EsrBwdPlan {
    size_t A, T, G[2], coef, bnslab, chan, part, part_b, part9, total;
};

int esr_bwd_plan(int N, int H, int W, int R, EsrBwdPlan& q) {
    EsrTrainPlan p;
    if (const int rc = esr_train_plan(N, H, W, R, p)) return rc;
    const size_t n = (size_t)N, t = n * 64 * H * W * sizeof(float);
    const size_t strips = ((size_t)H * W + D_BN_STRIP - 1) / D_BN_STRIP;
    size_t at = 0;
    q.A = take(at, t);
    q.T = take(at, t);
    q.G[0] = take(at, R ? t : 0);
    q.G[1] = take(at, R ? t : 0);
    q.coef = take(at, (size_t)64 * D_COEF * sizeof(float));
    q.bnslab = take(at, (size_t)64 * 3 * n * strips * sizeof(double));
    q.chan = take(at, 64 * sizeof(double));
    q.part = take(at, (size_t)kSrWgSplits * 4 * 64 * 144 * sizeof(float));
    q.part_b = take(at, (size_t)kSrWgSplits * 64 * sizeof(double));
    q.part9 = take(at, (size_t)std::max(kSrW9Splits, kSrTwSplits) * 64 * SG_W9_K * sizeof(double));
    q.total = at;
    return CID_OK;
}

}  // namespace

extern "C" {

int cid_esr_saved_bytes(int N, int H, int W, int num_residuals, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    EsrSavedPlan q;
    return plan_bytes(esr_saved_plan(N, H, W, num_residuals, q), q, bytes);
}

int cid_esr_forward_saved(cid_esr_t h, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, void* saved,
                          size_t saved_bytes, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_esr_forward_saved", stream);
    if (!saved) return cx.fail(CID_ERR_INVALID, "null pointer");
    EsrTrainPlan p;
    if (const int rc = esr_train_check(cx, h, in, in_fmt, out, CID_FMT_F32_NCHW, N, H, W, bn, workspace, p)) return rc;
    EsrSavedPlan q;
    esr_saved_plan(N, H, W, h->R, q);
    if (const int rc = cx.room(saved, saved_bytes, q.total, "cid_esr_saved_bytes", "saved buffer")) return rc;
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_esr_train_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    const int R = h->R;
    const EsrSavedBufs sv = esr_saved_bufs(saved, R, q);
    EsrTrainBufs b = esr_train_bufs(workspace, R, p);   // x1 and the slab stay in the workspace
    for (int l = 0; l < 2 * R; ++l) {
        b.z[l] = sv.z[l];
        b.st[l] = sv.st + l * 128;
        b.mi[l] = sv.mi + l * 128;
    }
    for (int i = 0; i + 1 < R; ++i) b.r[i] = sv.r[i];
    b.tail_in = sv.tail_in;
    b.v0 = sv.v0;
    return esr_train_run(cx, h, in, in_fmt, out, CID_FMT_F32_NCHW, N, H, W, bn, p, b);
}

int cid_esr_backward_workspace_bytes(int N, int H, int W, int num_residuals, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    EsrBwdPlan q;
    return plan_bytes(esr_bwd_plan(N, H, W, num_residuals, q), q, bytes);
}

int cid_esr_backward(cid_esr_t h, const void* in, int in_fmt, const float* grad_out, int N, int H, int W, const cid_disc_bn* bn,
                     const void* saved, size_t saved_bytes, const cid_esr_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_esr_backward", stream);
    const int R = h->R, L = 2 * R;
    if (!in || !grad_out || (R > 0 && !bn) || !saved || !g || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (!fmt_ok(in, in_fmt)) return cx.fail(CID_ERR_INVALID, "unknown format or misaligned fp32 operand");
    if ((uintptr_t)grad_out & 3) return cx.fail(CID_ERR_INVALID, "misaligned grad_out");
    for (int l = 0; l < L; ++l)
        if (!bn[l].gamma) return cx.fail(CID_ERR_INVALID, "null BatchNorm pointer");
    static_assert(sizeof(cid_esr_grads) % sizeof(float*) == 0, "pointers only");
    for (size_t i = 0; i < sizeof(cid_esr_grads) / sizeof(float*); ++i)
        if ((uintptr_t)reinterpret_cast<float* const*>(g)[i] & 3) return cx.fail(CID_ERR_INVALID, "misaligned gradient tensor");
    EsrSavedPlan sp;
    if (esr_saved_plan(N, H, W, R, sp) != CID_OK) return esr_train_shape_fail(cx, N, H, W);
    if (const int rc = cx.room(saved, saved_bytes, sp.total, "cid_esr_saved_bytes", "saved buffer")) return rc;
    EsrBwdPlan q;
    esr_bwd_plan(N, H, W, R, q);
    if (const int rc = cx.room(workspace, workspace_bytes, q.total, "cid_esr_backward_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;

    const hipStream_t s = cx.s;
    const EsrSavedBufs sv = esr_saved_bufs(const_cast<void*>(saved), R, sp);
    char* ws = static_cast<char*>(workspace);
    float* A = reinterpret_cast<float*>(ws + q.A);
    float* T = reinterpret_cast<float*>(ws + q.T);
    float* G[2] = {reinterpret_cast<float*>(ws + q.G[0]), reinterpret_cast<float*>(ws + q.G[1])};
    float* coef = reinterpret_cast<float*>(ws + q.coef);
    double* bnslab = reinterpret_cast<double*>(ws + q.bnslab);
    double* chan = reinterpret_cast<double*>(ws + q.chan);
    float* part = reinterpret_cast<float*>(ws + q.part);
    double* part_b = reinterpret_cast<double*>(ws + q.part_b);
    double* part9 = reinterpret_cast<double*>(ws + q.part9);
    const float* blob = h->dev_blob;
    const float* head_slope = blob + E_HEAD_K * 64 + 64;
    const float* tail_w = blob + kEsrHeadSeg + (size_t)L * kEsrConvSeg;
    const auto conv_seg = [&](int l) { return blob + kEsrHeadSeg + (size_t)l * kEsrConvSeg; };
    const auto block_slope = [&](int i) { return conv_seg(2 * i) + E_CONV_SLOPE; };
    const dim3 block(D_THREADS);
    const long long P = (long long)H * W;
    const int strips = (int)((P + D_BN_STRIP - 1) / D_BN_STRIP);
    const long long rows = (long long)N * strips;

    const SrgLaunch lx{cx, N, coef, bnslab, chan, part, part_b, part9};
    // ---- final: bias, weights, and the gradient of tail_in -> A.  The output is the raw sum: grad_out is taken as it is (raw = 1) and
    // the kernels do not read `out`.
    if (g->final_b) {
        if (const int rc = cx.launches(N, "final bias", [&](int n0, int n) {
            const SrgTailBiasArgs a{grad_out, nullptr, bnslab, rows, P, strips, 1, n0};
            hipLaunchKernelGGL(k_srg_tail_bias_part, dim3((unsigned)strips, (unsigned)n), block, 0, s, a);
        })) return rc;
        hipLaunchKernelGGL(k_srg_sum, dim3(3), block, 0, s, bnslab, rows, g->final_b);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("final bias");
    }
    if (g->final_w) {
        const int tiles_x = (W + D_TW - 1) / D_TW, tiles = ((H + D_WG_TH - 1) / D_WG_TH) * tiles_x;
        const long long items = (long long)N * tiles;
        const int splits = (int)std::min<long long>(items, kSrTwSplits);
        const SrgTailWgradArgs a{sv.tail_in, nullptr, grad_out, nullptr, part9, items, splits, H, W, tiles_x, tiles, 1};
        hipLaunchKernelGGL(k_srg_tail_wgrad<false>, dim3((unsigned)splits), block, 0, s, a);
        if (const int rc = lx.reduce9(g->final_w, nullptr, splits, 0, "final wgrad")) return rc;
    }
    {
        const int tiles_x = (W + D_TW - 1) / D_TW, tiles = ((H + 15) / 16) * tiles_x;
        if (const int rc = cx.launches(N, "final dgrad", [&](int n0, int n) {
            const SrgTailDgradArgs a{grad_out, nullptr, tail_w, A, H, W, tiles_x, 1, n0};
            hipLaunchKernelGGL(k_srg_tail_dgrad, dim3((unsigned)tiles, (unsigned)n), block, 0, s, a);
        })) return rc;
    }
    // ---- the blocks, last first.  Gi is the gradient of r_i; the outer skip gives G_{R-1} = dT.
    const float* Gi = A;
    int gc = 0;
    for (int i = R - 1; i >= 0; --i) {
        const int l1 = 2 * i + 1, l0 = 2 * i;
        // convolution 2i+1 and its BatchNorm, which no PReLU follows (coef slot 7 = 1): the gradient of PReLU_i's output -> T
        {
            const SrgDz dz{sv.z[l1], Gi, coef};
            if (const int rc = lx.slope_sums(k_srg_bn_part<SG_DZ_BN>, dz, sv.st + l1 * 128, sv.mi + l1 * 128, nullptr, bn[l1].gamma, g->gamma[l1],
                                          g->beta[l1], nullptr, H, W, "bn sums"))
                return rc;
            if (const int rc = lx.wgrad(k_srg_wgrad<SG_DZ_BN, SG_IN_BN_PRELU>, 1, dz, sv.z[l0], sv.st + l0 * 128, block_slope(i), g->conv_w[l1],
                                     g->conv_b[l1], H, W, "wgrad"))
                return rc;
            if (const int rc = lx.dgrad(k_srg_dgrad<64, SG_DZ_BN>, dz, conv_seg(l1), T, nullptr, H, W, "dgrad")) return rc;
        }
        // convolution 2i and its BatchNorm with the block's PReLU behind it; the block's skip: G_{i-1} = G_i + dgrad
        const SrgDz dz{sv.z[l0], T, coef};
        if (const int rc = lx.slope_sums(k_srg_bn_part<SG_DZ_BN>, dz, sv.st + l0 * 128, sv.mi + l0 * 128, block_slope(i), bn[l0].gamma, g->gamma[l0],
                                      g->beta[l0], g->slope[i], H, W, "bn sums"))
            return rc;
        const int rc = i == 0 ? lx.wgrad(k_srg_wgrad<SG_DZ_BN, SG_IN_PRELU>, 1, dz, sv.v0, nullptr, head_slope, g->conv_w[l0], g->conv_b[l0], H, W, "wgrad")
                              : lx.wgrad(k_srg_wgrad<SG_DZ_BN, SG_IN_RAW>, 1, dz, sv.r[i - 1], nullptr, nullptr, g->conv_w[l0], g->conv_b[l0], H, W, "wgrad");
        if (rc) return rc;
        if (const int rc2 = lx.dgrad(k_srg_dgrad<64, SG_DZ_BN>, dz, conv_seg(l0), G[gc], Gi, H, W, "dgrad")) return rc2;
        Gi = G[gc];
        gc = 1 - gc;
    }
    // ---- x1: d x1 = G_{-1} + dT -> T (R = 0: dT + dT)
    if (!g->head_slope && !g->head_w && !g->head_b) return CID_OK;
    if (const int rc = cx.launches(N, "join", [&](int n0, int n) {
        const EsrgJoinArgs a{R ? Gi : nullptr, A, T, 16 * P, n0};
        hipLaunchKernelGGL(k_esrg_join, dim3((unsigned)((16 * P + D_THREADS - 1) / D_THREADS), (unsigned)n), block, 0, s, a);
    })) return rc;
    // ---- head
    const SrgDz dz0{sv.v0, T, head_slope};
    if (g->head_slope)
        if (const int rc = lx.slope_sums(k_srg_bn_part<SG_DZ_PRELU>, dz0, nullptr, nullptr, head_slope, nullptr, nullptr, nullptr, g->head_slope,
                                      H, W, "head slope"))
            return rc;
    if (!g->head_w && !g->head_b) return CID_OK;
    const int segs = (W + SG_W9_PX - 1) / SG_W9_PX;
    const long long items = (long long)N * H * segs;
    const int splits = (int)std::min<long long>(items, kSrW9Splits);
    const SrgWgrad9Args a9{dz0, in, part9, items, splits, segs, H, W, in_fmt == CID_FMT_U8_NHWC};
    hipLaunchKernelGGL(k_srg_wgrad243<true>, dim3((unsigned)splits), block, 0, s, a9);
    return lx.reduce9(g->head_w, g->head_b, splits, 1, "head wgrad");
}

int cid_esr_pack_weights_device(cid_esr_t h, const float* const* dev_params, const cid_disc_bn* bn, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const int R = h->R, L = 2 * R;
    if (!dev_params || (R > 0 && !bn) || !device_blob) return h->fail(CID_ERR_INVALID, "cid_esr_pack_weights_device: null pointer");
    const int count = 3 + 9 * R + 2;
    for (int i = 0; i < count; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3))
            return h->fail(CID_ERR_INVALID, "cid_esr_pack_weights_device: null or misaligned parameter pointer");
    for (int l = 0; l < L; ++l) {
        if (!bn[l].gamma || !bn[l].beta || !bn[l].running_mean || !bn[l].running_var)
            return h->fail(CID_ERR_INVALID, "cid_esr_pack_weights_device: null BatchNorm pointer");
        if (!disc_finite_nonneg(bn[l].eps)) return h->fail(CID_ERR_INVALID, "cid_esr_pack_weights_device: eps must be finite and >= 0");
    }
    if ((uintptr_t)device_blob & 255) return h->fail(CID_ERR_WORKSPACE, "cid_esr_pack_weights_device: blob must be 256-byte aligned");
    static_assert(SG_PACK_HEAD == (int)kEsrHeadSeg && SG_PACK_CONV == (int)kEsrConvSeg && SG_PACK_TAIL == (int)kEsrTailSeg, "the segments of esr_pack");
    static_assert(2 * kEsrMaxBlocks == E_TRAIN_MAX_BNS, "k_esrg_pack holds every convolution's pointers");
    // dev_params in the module's parameter order: initial.0.{weight,bias}, initial.1.weight, per block block.0.{w,b} block.1.{w,b}
    // block.2.w block.3.{w,b} block.4.{w,b}, final.{w,b}
    EsrgPackArgs a{};
    const float* const* p = dev_params;
    a.head_w = p[0], a.head_b = p[1], a.head_slope = p[2];
    p += 3;
    for (int i = 0; i < R; ++i, p += 9) {
        a.conv_w[2 * i] = p[0], a.conv_b[2 * i] = p[1];
        a.slope[i] = p[4];
        a.conv_w[2 * i + 1] = p[5], a.conv_b[2 * i + 1] = p[6];
    }
    a.tail_w = p[0], a.tail_b = p[1];
    for (int l = 0; l < L; ++l) {
        a.gamma[l] = static_cast<const float*>(bn[l].gamma), a.beta[l] = static_cast<const float*>(bn[l].beta);
        a.mean[l] = static_cast<const float*>(bn[l].running_mean), a.var[l] = static_cast<const float*>(bn[l].running_var);
        a.eps[l] = bn[l].eps;
    }
    a.blob = static_cast<float*>(device_blob);
    a.R = R;
    const int longest = std::max({SG_PACK_HEAD, SG_PACK_CONV, SG_PACK_TAIL});
    hipLaunchKernelGGL(k_esrg_pack, dim3((longest + D_THREADS - 1) / D_THREADS, L + 2), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return h->fail(CID_ERR_HIP, "cid_esr_pack_weights_device: launch failed");
    h->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_esr_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int num_residuals, unsigned char* const* masks,
                        void* stream) {
    if (!saved || !masks) return CID_ERR_INVALID;
    EsrSavedPlan sp;
    if (const int rc = esr_saved_plan(N, H, W, num_residuals, sp)) return rc;
    for (int i = 0; i < 1 + num_residuals; ++i)
        if (!masks[i]) return CID_ERR_INVALID;
    if (saved_bytes < sp.total || ((uintptr_t)saved & 255)) return CID_ERR_WORKSPACE;
    const EsrSavedBufs sv = esr_saved_bufs(const_cast<void*>(saved), num_residuals, sp);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const long long P = (long long)H * W;
    for (int i = 0; i < 1 + num_residuals; ++i) {   // the head on v0, block i - 1 on BN(z_{2(i-1)})
        const DiscMaskArgs a{i == 0 ? sv.v0 : sv.z[2 * (i - 1)], i == 0 ? nullptr : sv.st + 2 * (i - 1) * 128, masks[i], (long long)N * 64 * P, P, 64};
        const long long blocks = (a.total + D_THREADS - 1) / D_THREADS;
        if (blocks > 0x7fffffffLL) return CID_ERR_SHAPE;
        hipLaunchKernelGGL(k_disc_masks, dim3((unsigned)blocks), dim3(D_THREADS), 0, s, a);
        if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
    }
    return CID_OK;
}

}  // extern "C"
