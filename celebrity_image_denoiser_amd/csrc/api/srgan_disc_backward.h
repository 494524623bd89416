// The SRGAN trainer's discriminator: saved forward, backward pass, device pack and masks (cid_srd_*).  The head's kernels are in
// srgan_disc_bwd_kernels.h; BatchNorm 12 and model.11 run on instantiations of disc_bwd_kernels.h, everything below on the stages the
// denoise discriminator's backward shares (disc_bwd_lower, disc_backward.h).  Host code.
#pragma once
#include "../srgan_disc_bwd_kernels.h"
#include "disc_backward.h"
#include "srgan_disc.h"

namespace {

// Workspace of one backward call.  Y holds the gradient of a9 (model.11's data gradient), later of a3; X the gradient of a6, later of
// a0.  model.11's launches: the weight gradient keeps 128 dz channels per workgroup (grid z = half), the data gradient tiles like the
// forward's layer 11.
struct SrdBwdPlan : DiscBwdTiling {
    int strips11, wg11_tiles_x, wg11_tiles, wg11_splits, dg11_tiles_x, dg11_tiles;
    size_t dl, dh, up, total;
};

constexpr int kSrdDg11TileRows = DiscDgradGeom<256, 128, 1>::TH;

void srd_bwd_plan(int N, const DiscPlan& p, SrdBwdPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    const int H = p.H, W = p.W;
    disc_bwd_tiling(kSrdNet, N, p, q);
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
    q.coef = take(at, (size_t)kSrdNet.nbn * kSrdNet.maxc * D_COEF * f);
    q.bnslab = take(at, std::max(q.max_bnslab, (size_t)256 * 2 * n * q.strips11 * sizeof(double)));
    q.X = take(at, std::max(n * 128 * p.H2 * p.W2, n * 64 * H * W) * f);
    q.Y = take(at, std::max(n * 64 * p.H2 * p.W2, n * 128 * p.H4 * p.W4) * f);
    q.part = take(at, std::max(q.max_part, (size_t)q.wg11_splits * 128 * 256 * 9 * f));
    q.part_b = take(at, std::max(q.max_part_b, (size_t)q.wg11_splits * 256 * sizeof(double)));
    q.part0 = take(at, (size_t)q.w0_splits * 64 * 28 * sizeof(double));
    q.total = at;
}

}  // namespace

extern "C" {

int cid_srd_saved_bytes(int N, int H, int W, int training, size_t* bytes) { return disc_saved_bytes(kSrdNet, N, H, W, training, bytes); }

int cid_srd_forward_saved(cid_srd_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, int training,
                          void* saved, size_t saved_bytes, void* stream) {
    return disc_forward(d, "cid_srd_forward_saved", in, in_fmt, out, N, H, W, bn, training, saved, saved_bytes, true, stream,
                        srd_top_launches);
}

int cid_srd_backward_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    SrdBwdPlan q;
    const int rc = disc_plan(kSrdNet, N, H, W, training, p);
    if (rc == CID_OK) srd_bwd_plan(N, p, q);
    return plan_bytes(rc, q, bytes);
}

int cid_srd_backward(cid_srd_t d, const void* in, int in_fmt, const float* grad_prob, int N, int H, int W, const cid_disc_bn* bn,
                     int training, const void* saved, size_t saved_bytes, const cid_srd_grads* grads, void* workspace, size_t workspace_bytes,
                     void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, "cid_srd_backward", stream);
    const DiscGrads g = disc_grads(grads);
    DiscPlan p;
    DiscBufs sv;
    if (const int rc = disc_bwd_prepare(cx, kSrdNet, in, in_fmt, grad_prob, N, H, W, bn, training, saved, saved_bytes, grads, g, workspace, p, sv))
        return rc;
    SrdBwdPlan q;
    srd_bwd_plan(N, p, q);
    if (const int rc = cx.room(workspace, workspace_bytes, q.total, "cid_srd_backward_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;

    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    double* dl = reinterpret_cast<double*>(ws + q.dl);
    double* dh = reinterpret_cast<double*>(ws + q.dh);
    float* up = reinterpret_cast<float*>(ws + q.up);
    float* coef11 = reinterpret_cast<float*>(ws + q.coef) + 3 * kSrdNet.maxc * D_COEF;
    const float* blob = d->dev_blob;
    const size_t* off = kSrdNet.off;
    const DiscBwdLower c = disc_bwd_lower_args(cx, kSrdNet, in, in_fmt, N, p, training, bn, sv, g, workspace, q);
    const float* z11 = sv.z[4];

    // stages above the shared chain: head (model.15, model.17) > bn12 > conv11
    const bool lower = c.wanted();   // something below model.11 is asked for
    const bool want_head = g.w[5] || g.b[5] || g.w[6] || g.b[6];
    const bool want_bn12 = g.gamma[3] || g.beta[3], want_conv11 = g.w[4] || g.b[4];
    if (!(want_head || want_bn12 || want_conv11 || lower)) return CID_OK;
    const long long P4 = (long long)p.H4 * p.W4;

    // head
    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        SrdHeadBwdArgs a{sv.hidden, blob + off[5], blob + off[6], grad_prob, dl, dh, up, (double)P4, n0};
        hipLaunchKernelGGL(k_srd_head_bwd, dim3((unsigned)n), dim3(SRD_HB_THREADS), 0, s, a);
    })) return rc;
    if (want_head) {
        SrdHeadReduceArgs a{sv.pooled, sv.hidden, dl, dh, g.w[5], g.b[5], g.w[6], g.b[6], N};
        hipLaunchKernelGGL(k_srd_head_reduce, dim3(SRD_HR_BLOCKS + 1), dim3(SRD_HEAD_C), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("head reduce");
    }
    if (!(want_bn12 || want_conv11 || lower)) return CID_OK;

    // BN12: the upstream gradient of a12 is up[n][c] at every pixel
    if (disc_bn_part_launch<256, false, true>(disc_bn_part_args(z11, nullptr, up, coef11, sv.st[3], sv.mi[3], c.bnslab, N, q.strips11, P4),
                                              N, s) != hipSuccess)
        return cx.hip("bn12 sums");
    if (disc_bn_reduce_launch(256, c.bnslab, (long long)N * q.strips11, (double)N * (double)P4, bn[3], sv.st[3], sv.mi[3], training, coef11,
                              g.gamma[3], g.beta[3], s) != hipSuccess)
        return cx.hip("bn12 reduce");
    if (!(want_conv11 || lower)) return CID_OK;
    // layer 11
    const DiscDzSrc dz11{z11, nullptr, up, coef11};
    if (want_conv11 &&
        disc_wgrad_launch<kSrdHalf, 128, 1, true, false, true, 256>(
            disc_wgrad_args(dz11, c.z8, sv.st[2], c.part, c.part_b, N, q.wg11_tiles_x, q.wg11_tiles, q.wg11_splits, p.H4, p.W4, p.H4, p.W4),
            g.w[4], g.b[4], s) != hipSuccess)
        return cx.hip("wgrad11");
    if (!lower) return CID_OK;
    if (disc_dgrad_launch<256, 128, 1, false, true, kSrdHalf>(
            disc_dgrad_args(dz11, blob + off[4], c.Y, q.dg11_tiles_x, p.H4, p.W4, p.H4, p.W4), q.dg11_tiles, N, s) != hipSuccess)
        return cx.hip("dgrad11");
    // BatchNorm 9 and below: the denoise discriminator's stages, BatchNorm 9's upstream being the tensor in Y
    return disc_bwd_lower<false>(cx, c, q, c.Y, nullptr);
}

int cid_srd_pack_weights_device(cid_srd_t d, const float* const* dev_params, void* device_blob, void* stream) {
    static_assert(CID_SRD_NUM_WEIGHTS == 2 * kSrdNet.nconv, "a weight and a bias per convolution");
    return disc_pack_weights_device(d, dev_params, device_blob, stream);
}

int cid_srd_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int training, unsigned char* const* masks, void* stream) {
    DiscBufs sv;
    if (const int rc = disc_saved_masks(kSrdNet, saved, saved_bytes, N, H, W, training, masks, kSrdNet.nbn + 2, stream, sv)) return rc;
    // the hidden layer's mask, after the shared ones
    const long long total = (long long)N * SRD_HEAD_HID;
    hipLaunchKernelGGL(k_srd_hidden_mask, dim3((unsigned)((total + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0,
                       static_cast<hipStream_t>(stream), sv.hidden, masks[kSrdNet.nbn + 1], total);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
