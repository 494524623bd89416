// The SRGAN trainer's discriminator: saved forward, backward pass, device pack and masks (cid_srd_*).  The head's kernels are in
// srgan_disc_bwd_kernels.h; BatchNorm 12 and model.11 run on instantiations of disc_bwd_kernels.h, everything below on the stages the
// denoise discriminator's backward shares (disc_bwd_lower, disc_backward.h).  Host code.
#pragma once
#include "../srgan_disc_bwd_kernels.h"
#include "disc_backward.h"
#include "srgan_disc.h"

namespace {

// What cid_srd_forward_saved keeps for one call.
struct SrdSavedPlan {
    size_t a0, z2, z5, z8, z11, st, mi, pooled, hidden, slab[SRD_BNS], total;
};

void srd_saved_plan(int N, int H, int W, int training, const SrdPlan& p, SrdSavedPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    size_t at = 0;
    q.a0 = take(at, n * 64 * H * W * f);
    q.z2 = take(at, n * 64 * p.H2 * p.W2 * f);
    q.z5 = take(at, n * 128 * p.H2 * p.W2 * f);
    q.z8 = take(at, n * 128 * p.H4 * p.W4 * f);
    q.z11 = take(at, n * 256 * p.H4 * p.W4 * f);
    q.st = take(at, (size_t)SRD_BNS * SRD_BN_MAXC * 2 * f);
    q.mi = take(at, (size_t)SRD_BNS * SRD_BN_MAXC * 2 * sizeof(double));
    q.pooled = take(at, n * SRD_HEAD_C * sizeof(double));
    q.hidden = take(at, n * SRD_HEAD_HID * sizeof(double));
    for (int l = 0; l < SRD_BNS; ++l) q.slab[l] = training ? take(at, (size_t)kSrdBnC[l] * 2 * n * p.tiles[l] * sizeof(double)) : at;
    q.total = at;
}

SrdBufs srd_saved_bufs(void* saved, const SrdSavedPlan& q) {
    char* sv = static_cast<char*>(saved);
    SrdBufs b{};
    b.a0 = reinterpret_cast<float*>(sv + q.a0);
    b.z2 = reinterpret_cast<float*>(sv + q.z2);
    b.z5 = reinterpret_cast<float*>(sv + q.z5);
    b.z8 = reinterpret_cast<float*>(sv + q.z8);
    b.z11 = reinterpret_cast<float*>(sv + q.z11);
    for (int l = 0; l < SRD_BNS; ++l) {
        b.st[l] = reinterpret_cast<float*>(sv + q.st) + l * SRD_BN_MAXC * 2;
        b.mi[l] = reinterpret_cast<double*>(sv + q.mi) + l * SRD_BN_MAXC * 2;
        b.slab[l] = reinterpret_cast<double*>(sv + q.slab[l]);
    }
    b.pooled = reinterpret_cast<double*>(sv + q.pooled);
    b.hidden = reinterpret_cast<double*>(sv + q.hidden);
    return b;
}

// Workspace of one backward call.  Y holds the gradient of a9 (model.11's data gradient), later of a3; X the gradient of a6, later of
// a0.  model.11's launches: the weight gradient keeps 128 dz channels per workgroup (grid z = half), the data gradient tiles like the
// forward's layer 11.
struct SrdBwdPlan : DiscBwdTiling {
    int strips11, wg11_tiles_x, wg11_tiles, wg11_splits, dg11_tiles_x, dg11_tiles;
    size_t dl, dh, up, coef, bnslab, X, Y, part, part_b, part0, total;
};

constexpr int kSrdDg11TileRows = DiscDgradGeom<256, 128, 1>::TH;

void srd_bwd_plan(int N, int H, int W, const SrdPlan& p, SrdBwdPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    disc_bwd_tiling(N, H, W, p, q);
    q.strips11 = (int)(((long long)p.H4 * p.W4 + D_BN_STRIP - 1) / D_BN_STRIP);
    q.wg11_tiles_x = (p.W4 + D_TW - 1) / D_TW;
    q.wg11_tiles = ((p.H4 + D_WG_TH - 1) / D_WG_TH) * q.wg11_tiles_x;
    q.wg11_splits = (int)std::min<long long>((long long)N * q.wg11_tiles, 512 / (128 / 16));
    q.dg11_tiles_x = (p.W4 + D_TW - 1) / D_TW;
    q.dg11_tiles = ((p.H4 + kSrdDg11TileRows - 1) / kSrdDg11TileRows) * q.dg11_tiles_x;
    size_t at = 0;
    q.dl = take(at, n * sizeof(double));
    q.dh = take(at, n * SRD_HEAD_HID * sizeof(double));
    q.up = take(at, n * SRD_HEAD_C * f);
    q.coef = take(at, (size_t)SRD_BNS * SRD_BN_MAXC * D_COEF * f);
    q.bnslab = take(at, std::max(q.max_bnslab, (size_t)256 * 2 * n * q.strips11 * sizeof(double)));
    q.X = take(at, std::max(n * 128 * p.H2 * p.W2, n * 64 * H * W) * f);
    q.Y = take(at, std::max(n * 64 * p.H2 * p.W2, n * 128 * p.H4 * p.W4) * f);
    q.part = take(at, std::max(q.max_part, (size_t)q.wg11_splits * 128 * 256 * 9 * f));
    q.part_b = take(at, std::max(q.max_part_b, (size_t)q.wg11_splits * 256 * sizeof(double)));
    q.part0 = take(at, (size_t)q.w0_splits * 64 * 28 * sizeof(double));
    q.total = at;
}

int srd_bwd_shape(const Call& cx, int N, int H, int W, int training, SrdPlan& p) {
    if (training != 0 && training != 1) return cx.fail(CID_ERR_INVALID, "training must be 0 or 1");
    if (srd_plan(N, H, W, training, p) != CID_OK)
        return cx.fail(CID_ERR_SHAPE, "shape not accepted (N, H, W >= 1, H*W < 2^31, more than one value per channel in train mode)");
    return CID_OK;
}

}  // namespace

extern "C" {

int cid_srd_saved_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    SrdPlan p;
    SrdSavedPlan q;
    const int rc = srd_plan(N, H, W, training, p);
    if (rc == CID_OK) srd_saved_plan(N, H, W, training, p, q);
    return plan_bytes(rc, q, bytes);
}

int cid_srd_forward_saved(cid_srd_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, int training,
                          void* saved, size_t saved_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, "cid_srd_forward_saved", stream);
    SrdPlan p;
    if (const int rc = disc_check_args(cx, in, in_fmt, out, N, H, W, bn, SRD_BNS, training, saved,
                                       [&] { return srd_plan(N, H, W, training, p); }))
        return rc;
    SrdSavedPlan q;
    srd_saved_plan(N, H, W, training, p, q);
    if (const int rc = cx.room(saved, saved_bytes, q.total, "cid_srd_saved_bytes", "saved buffer")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    return srd_forward_run(cx, in, in_fmt, out, N, H, W, bn, training, p, srd_saved_bufs(saved, q));
}

int cid_srd_backward_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    SrdPlan p;
    SrdBwdPlan q;
    const int rc = srd_plan(N, H, W, training, p);
    if (rc == CID_OK) srd_bwd_plan(N, H, W, p, q);
    return plan_bytes(rc, q, bytes);
}

int cid_srd_backward(cid_srd_t d, const void* in, int in_fmt, const float* grad_prob, int N, int H, int W, const cid_disc_bn* bn,
                     int training, const void* saved, size_t saved_bytes, const cid_srd_grads* g, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, "cid_srd_backward", stream);
    if (const int rc = disc_bwd_check_args(cx, in, in_fmt, grad_prob, bn, SRD_BNS, saved, g, workspace, g ? g->w : nullptr,
                                           g ? g->b : nullptr, kSrdConvs, g ? g->gamma : nullptr, g ? g->beta : nullptr,
                                           g ? g->input : nullptr))
        return rc;
    SrdPlan p;
    if (const int rc = srd_bwd_shape(cx, N, H, W, training, p)) return rc;
    SrdSavedPlan sp;
    srd_saved_plan(N, H, W, training, p, sp);
    if (const int rc = cx.room(saved, saved_bytes, sp.total, "cid_srd_saved_bytes", "saved buffer")) return rc;
    SrdBwdPlan q;
    srd_bwd_plan(N, H, W, p, q);
    if (const int rc = cx.room(workspace, workspace_bytes, q.total, "cid_srd_backward_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;

    const hipStream_t s = cx.s;
    const SrdBufs sv = srd_saved_bufs(const_cast<void*>(saved), sp);
    char* ws = static_cast<char*>(workspace);
    double* dl = reinterpret_cast<double*>(ws + q.dl);
    double* dh = reinterpret_cast<double*>(ws + q.dh);
    float* up = reinterpret_cast<float*>(ws + q.up);
    float* coef11 = reinterpret_cast<float*>(ws + q.coef) + 3 * SRD_BN_MAXC * D_COEF;
    const float* blob = d->dev_blob;
    DiscBwdLower c{};
    c.in = in;
    c.in_fmt = in_fmt;
    c.N = N, c.H = H, c.W = W, c.H2 = p.H2, c.W2 = p.W2, c.H4 = p.H4, c.W4 = p.W4;
    c.training = training;
    c.bn = bn;
    c.a0 = sv.a0, c.z2 = sv.z2, c.z5 = sv.z5, c.z8 = sv.z8;
    c.st = sv.st;
    c.mi = sv.mi;
    bool lower = g->input != nullptr;   // something below model.11 is asked for
    for (int i = 0; i < 4; ++i) {
        c.w[i] = blob + kSrdBlob.off[i];
        c.gw[i] = g->w[i];
        c.gb[i] = g->b[i];
        lower = lower || g->w[i] || g->b[i];
    }
    for (int l = 0; l < 3; ++l) {
        c.ggamma[l] = g->gamma[l];
        c.gbeta[l] = g->beta[l];
        c.coef[l] = reinterpret_cast<float*>(ws + q.coef) + l * SRD_BN_MAXC * D_COEF;
        lower = lower || g->gamma[l] || g->beta[l];
    }
    c.ginput = g->input;
    c.bnslab = reinterpret_cast<double*>(ws + q.bnslab);
    c.X = reinterpret_cast<float*>(ws + q.X);
    c.Y = reinterpret_cast<float*>(ws + q.Y);
    c.part = reinterpret_cast<float*>(ws + q.part);
    c.part_b = reinterpret_cast<double*>(ws + q.part_b);
    c.part0 = reinterpret_cast<double*>(ws + q.part0);

    // stages above the shared chain: head (model.15, model.17) > bn12 > conv11
    const bool want_head = g->w[5] || g->b[5] || g->w[6] || g->b[6];
    const bool want_bn12 = g->gamma[3] || g->beta[3], want_conv11 = g->w[4] || g->b[4];
    if (!(want_head || want_bn12 || want_conv11 || lower)) return CID_OK;
    const long long P4 = (long long)p.H4 * p.W4;

    // head
    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        SrdHeadBwdArgs a{sv.hidden, blob + kSrdBlob.off[5], blob + kSrdBlob.off[6], grad_prob, dl, dh, up, (double)P4, n0};
        hipLaunchKernelGGL(k_srd_head_bwd, dim3((unsigned)n), dim3(SRD_HB_THREADS), 0, s, a);
    })) return rc;
    if (want_head) {
        SrdHeadReduceArgs a{sv.pooled, sv.hidden, dl, dh, g->w[5], g->b[5], g->w[6], g->b[6], N};
        hipLaunchKernelGGL(k_srd_head_reduce, dim3(SRD_HR_BLOCKS + 1), dim3(SRD_HEAD_C), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("head reduce");
    }
    if (!(want_bn12 || want_conv11 || lower)) return CID_OK;

    // BN12: the upstream gradient of a12 is up[n][c] at every pixel
    if (disc_bn_part_launch<256, false, true>(disc_bn_part_args(sv.z11, nullptr, up, coef11, sv.st[3], sv.mi[3], c.bnslab, N, q.strips11, P4),
                                              N, s) != hipSuccess)
        return cx.hip("bn12 sums");
    if (disc_bn_reduce_launch(256, c.bnslab, (long long)N * q.strips11, (double)N * (double)P4, bn[3], sv.st[3], sv.mi[3], training, coef11,
                              g->gamma[3], g->beta[3], s) != hipSuccess)
        return cx.hip("bn12 reduce");
    if (!(want_conv11 || lower)) return CID_OK;
    // layer 11
    const DiscDzSrc dz11{sv.z11, nullptr, up, coef11};
    if (want_conv11 &&
        disc_wgrad_launch<kSrdHalf, 128, 1, true, false, true, 256>(
            disc_wgrad_args(dz11, sv.z8, sv.st[2], c.part, c.part_b, N, q.wg11_tiles_x, q.wg11_tiles, q.wg11_splits, p.H4, p.W4, p.H4, p.W4),
            g->w[4], g->b[4], s) != hipSuccess)
        return cx.hip("wgrad11");
    if (!lower) return CID_OK;
    if (disc_dgrad_launch<256, 128, 1, false, true, kSrdHalf>(
            disc_dgrad_args(dz11, blob + kSrdBlob.off[4], c.Y, q.dg11_tiles_x, p.H4, p.W4, p.H4, p.W4), q.dg11_tiles, N, s) != hipSuccess)
        return cx.hip("dgrad11");
    // BatchNorm 9 and below: the denoise discriminator's stages, BatchNorm 9's upstream being the tensor in Y
    return disc_bwd_lower<false>(cx, c, q, c.Y, nullptr);
}

int cid_srd_pack_weights_device(cid_srd_t d, const float* const* dev_params, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    if (!dev_params || !device_blob) return d->fail(CID_ERR_INVALID, "cid_srd_pack_weights_device: null pointer");
    for (int i = 0; i < CID_SRD_NUM_WEIGHTS; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3))
            return d->fail(CID_ERR_INVALID, "cid_srd_pack_weights_device: null or misaligned parameter pointer");
    if ((uintptr_t)device_blob & 255) return d->fail(CID_ERR_WORKSPACE, "cid_srd_pack_weights_device: blob must be 256-byte aligned");
    static_assert(kSrdConvs == SRD_PACK_LAYERS, "one slot per convolution");
    SrdPackArgs a{};
    for (int i = 0; i < kSrdConvs; ++i) {
        const auto& L = kSrdConv[i];
        a.w[i] = dev_params[2 * i];
        a.b[i] = dev_params[2 * i + 1];
        a.off[i] = (int)kSrdBlob.off[i];
        a.cin[i] = L.cin;
        a.cout[i] = L.cout;
        a.kk[i] = L.k * L.k;
        a.part[i] = (L.k == 1 || i == 0) ? 0 : (i == 4 ? kSrdHalf : L.cout);
    }
    a.blob = static_cast<float*>(device_blob);
    a.total = (int)kSrdBlob.total;
    hipLaunchKernelGGL(k_srd_pack, dim3((a.total + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return d->fail(CID_ERR_HIP, "cid_srd_pack_weights_device: launch failed");
    d->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_srd_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int training, unsigned char* const* masks, void* stream) {
    if (!saved || !masks || (training != 0 && training != 1)) return CID_ERR_INVALID;
    for (int i = 0; i < 6; ++i)
        if (!masks[i]) return CID_ERR_INVALID;
    SrdPlan p;
    const int rc = srd_plan(N, H, W, training, p);
    if (rc != CID_OK) return rc;
    SrdSavedPlan sp;
    srd_saved_plan(N, H, W, training, p, sp);
    if (saved_bytes < sp.total || ((uintptr_t)saved & 255)) return CID_ERR_WORKSPACE;
    const SrdBufs sv = srd_saved_bufs(const_cast<void*>(saved), sp);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    const float* z[5] = {sv.a0, sv.z2, sv.z5, sv.z8, sv.z11};
    const float* st[5] = {nullptr, sv.st[0], sv.st[1], sv.st[2], sv.st[3]};
    const int C[5] = {64, 64, 128, 128, 256};
    const long long P2 = (long long)p.H2 * p.W2, P4 = (long long)p.H4 * p.W4;
    const long long P[5] = {(long long)H * W, P2, P2, P4, P4};
    for (int i = 0; i < 5; ++i) {
        DiscMaskArgs a{z[i], st[i], masks[i], (long long)N * C[i] * P[i], P[i], C[i]};
        const long long blocks = (a.total + D_THREADS - 1) / D_THREADS;
        if (blocks > 0x7fffffffLL) return CID_ERR_SHAPE;
        hipLaunchKernelGGL(k_disc_masks, dim3((unsigned)blocks), dim3(D_THREADS), 0, s, a);
        if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
    }
    const long long total = (long long)N * SRD_HEAD_HID;
    hipLaunchKernelGGL(k_srd_hidden_mask, dim3((unsigned)((total + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, s, sv.hidden, masks[5], total);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
