// The ESRGAN trainer's discriminator: saved forward, backward pass and device pack (cid_esd_*); kernels in
// esrgan_disc_bwd_kernels.h, the forward's plan and launches in esrgan_disc.h.  Host code.
#pragma once
#include "../esrgan_disc_bwd_kernels.h"
#include "esrgan_disc.h"

namespace {

// One MFMA layer's backward launches (index 0, 1, 2 = conv2, conv3, conv4).  CD: dz channels per weight-gradient workgroup; CXW, PT:
// input channels and class rows per wave of a data-gradient workgroup (DESIGN section 27 has the reasoning).
constexpr int kEsdWgCD[3] = {128, 128, 64};
constexpr int kEsdDgCXW[3] = {64, 128, 128}, kEsdDgPT[3] = {4, 4, 2};
constexpr int kEsdWgTarget = 256;   // workgroups a weight-gradient launch aims at
// Items one weight-gradient workgroup may add into its fp32 MFMA accumulators before the fp64 reduce takes over: the error of that
// chain grows with its length (measured at 65,537 one-pixel images: 9e-7 of max|dW| at 1,024 items, 3e-6 at 4,096, 6e-5 at 32,768).
constexpr long long kEsdWgMaxItems = 2048;

struct EsdBwdPlan {
    int wg_tiles_x[3], wg_tiles[3], wg_splits[3];
    int dg_tiles_x[3], dg_tiles[3];
    int w1_strips, w1_splits;
    size_t da[3], part, part_b, part1, total;   // gradients of a1, a2, a3; the partials
};

void esd_bwd_plan(int N, const EsdPlan& p, EsdBwdPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    const EsdDims& d = p.d;
    size_t max_part = 0, max_part_b = 0;
    for (int i = 0; i < 3; ++i) {
        const int l = i + 1;   // conv(l + 1): output ho[l] x wo[l], input ho[l - 1] x wo[l - 1]
        const int cd = kEsdConv[l].cout, cx = kEsdConv[l].cin;
        q.wg_tiles_x[i] = cdiv(d.wo[l], D_TW);
        q.wg_tiles[i] = cdiv(d.ho[l], D_WG_TH) * q.wg_tiles_x[i];
        const long long items = (long long)N * q.wg_tiles[i];
        const long long by_target = cdiv(kEsdWgTarget, (cx / 16) * (cd / kEsdWgCD[i])), by_length = (items + kEsdWgMaxItems - 1) / kEsdWgMaxItems;
        q.wg_splits[i] = (int)std::min(items, std::max(by_target, by_length));
        max_part = std::max(max_part, (size_t)q.wg_splits[i] * cd * cx * 9 * f);
        max_part_b = std::max(max_part_b, (size_t)q.wg_splits[i] * cd * sizeof(double));
        const int th = 4 / (kEsdDgCXW[i] / 64) * kEsdDgPT[i];
        q.dg_tiles_x[i] = cdiv(cdiv(d.wo[l - 1], 2), D_TW);
        q.dg_tiles[i] = cdiv(cdiv(d.ho[l - 1], 2), th) * q.dg_tiles_x[i];
    }
    q.w1_strips = (int)(((long long)d.ho[0] * d.wo[0] + 63) / 64);
    q.w1_splits = (int)std::min<long long>((long long)N * q.w1_strips, 256);   // k_disc_wgrad0_reduce walks them serially
    size_t at = 0;
    for (int l = 0; l < 3; ++l) q.da[l] = take(at, n * kEsdConv[l].cout * d.ho[l] * d.wo[l] * f);
    q.part = take(at, max_part);
    q.part_b = take(at, max_part_b);
    q.part1 = take(at, (size_t)q.w1_splits * 64 * 28 * sizeof(double));
    q.total = at;
}

template <int CD, int CX, bool FC>
hipError_t esd_wgrad_launch(const EsdWgradArgs& a, float* dw, float* db, hipStream_t s) {
    hipLaunchKernelGGL((k_esd_wgrad<CD, CX, FC>), dim3((unsigned)a.splits, CX / 16, (unsigned)(a.cd_total / CD)), dim3(D_THREADS), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const DiscWgradReduceArgs r{a.part, a.part_b, dw, db, a.splits, a.cd_total, CX};
    hipLaunchKernelGGL(k_disc_wgrad_reduce, dim3((a.cd_total * CX * 9 + a.cd_total + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, s, r);
    return hipGetLastError();
}

template <int CD, int CX, int CXW, int PT, bool FC>
hipError_t esd_dgrad_launch(const EsdDgradArgs& base, int tiles, int N, hipStream_t s) {
    static_assert(EsdDgradGeom<CXW, PT>::TH >= 1, "tile");
    (void)for_each_launch(N, [&](int n0, int n) {
        EsdDgradArgs a = base;
        a.n0 = n0;
        const dim3 grid((unsigned)tiles, (unsigned)n, 4 * (CX / CXW));
        hipLaunchKernelGGL((k_esd_dgrad<CD, CX, CXW, PT, FC>), grid, dim3(D_THREADS), 0, s, a);
    });
    return hipGetLastError();
}

// The checks cid_esd_forward and cid_esd_forward_saved share, then the launches; `buf` is the workspace or the saved buffer.
int esd_forward(cid_esd_t d, const char* fn, const void* in, int in_fmt, float* out_logit, int N, int H, int W, void* buf, size_t buf_bytes,
                const char* sizer, const char* noun, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, fn, stream);
    if (!in || !out_logit || !buf) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) return cx.fail(CID_ERR_INVALID, "unknown input format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || ((uintptr_t)out_logit & 3))
        return cx.fail(CID_ERR_INVALID, "misaligned fp32 operand");
    if (N < 1) return cx.fail(CID_ERR_SHAPE, "N >= 1 required");
    if (H != d->H || W != d->W) return cx.fail(CID_ERR_SHAPE, esd_size_message(d, H, W));
    EsdPlan p(H, W);
    if (esd_plan(N, H, W, p) != CID_OK) return cx.fail(CID_ERR_SHAPE, "input shape not accepted");
    if (const int rc = cx.room(buf, buf_bytes, p.total, sizer, noun)) return rc;
    if (const int rc = cx.uploaded()) return rc;
    return esd_forward_run(cx, *d, in, in_fmt, out_logit, N, p, static_cast<char*>(buf));
}

}  // namespace

extern "C" {

int cid_esd_forward(cid_esd_t d, const void* in, int in_fmt, float* out_logit, int N, int H, int W, void* workspace, size_t workspace_bytes,
                    void* stream) {
    return esd_forward(d, "cid_esd_forward", in, in_fmt, out_logit, N, H, W, workspace, workspace_bytes, "cid_esd_workspace_bytes", "workspace",
                       stream);
}

int cid_esd_saved_bytes(int N, int H, int W, size_t* bytes) { return cid_esd_workspace_bytes(N, H, W, bytes); }

int cid_esd_forward_saved(cid_esd_t d, const void* in, int in_fmt, float* out_logit, int N, int H, int W, void* saved, size_t saved_bytes,
                          void* stream) {
    return esd_forward(d, "cid_esd_forward_saved", in, in_fmt, out_logit, N, H, W, saved, saved_bytes, "cid_esd_saved_bytes", "saved buffer",
                       stream);
}

int cid_esd_backward_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    if (!esd_side_ok(H, W)) return CID_ERR_SHAPE;
    EsdPlan p(H, W);
    EsdBwdPlan q;
    const int rc = esd_plan(N, H, W, p);
    if (rc == CID_OK) esd_bwd_plan(N, p, q);
    return plan_bytes(rc, q, bytes);
}

int cid_esd_backward(cid_esd_t d, const void* in, int in_fmt, const float* grad_logit, int N, int H, int W, const void* saved,
                     size_t saved_bytes, const cid_esd_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, "cid_esd_backward", stream);
    if (!in || !grad_logit || !saved || !g || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) return cx.fail(CID_ERR_INVALID, "unknown input format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || ((uintptr_t)grad_logit & 3))
        return cx.fail(CID_ERR_INVALID, "misaligned fp32 operand");
    bool misaligned = ((uintptr_t)g->input & 3) != 0;
    for (int i = 0; i <= kEsdConvs; ++i) misaligned = misaligned || ((uintptr_t)g->w[i] & 3) || ((uintptr_t)g->b[i] & 3);
    if (misaligned) return cx.fail(CID_ERR_INVALID, "misaligned gradient pointer");
    if (g->input && in_fmt != CID_FMT_F32_NCHW) return cx.fail(CID_ERR_INVALID, "a uint8 input has no gradient (grads.input must be null)");
    if (N < 1) return cx.fail(CID_ERR_SHAPE, "N >= 1 required");
    if (H != d->H || W != d->W) return cx.fail(CID_ERR_SHAPE, esd_size_message(d, H, W));
    EsdPlan p(H, W);
    if (esd_plan(N, H, W, p) != CID_OK) return cx.fail(CID_ERR_SHAPE, "input shape not accepted");
    if (const int rc = cx.room(saved, saved_bytes, p.total, "cid_esd_saved_bytes", "saved buffer")) return rc;
    EsdBwdPlan q;
    esd_bwd_plan(N, p, q);
    if (const int rc = cx.room(workspace, workspace_bytes, q.total, "cid_esd_backward_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;

    const hipStream_t s = cx.s;
    const EsdDims& dm = p.d;
    const char* sv = static_cast<const char*>(saved);
    char* ws = static_cast<char*>(workspace);
    const float* a[kEsdConvs];
    for (int l = 0; l < kEsdConvs; ++l) a[l] = reinterpret_cast<const float*>(sv + p.a[l]);
    float* da[3];
    for (int l = 0; l < 3; ++l) da[l] = reinterpret_cast<float*>(ws + q.da[l]);
    float* part = reinterpret_cast<float*>(ws + q.part);
    double* part_b = reinterpret_cast<double*>(ws + q.part_b);
    double* part1 = reinterpret_cast<double*>(ws + q.part1);
    const float* blob = d->dev_blob;

    // what is asked for at each stage: fc(5) > conv4(4) > conv3(3) > conv2(2) > conv1(1) > input(0)
    const bool want[6] = {g->input != nullptr, g->w[0] || g->b[0], g->w[1] || g->b[1], g->w[2] || g->b[2], g->w[3] || g->b[3],
                          g->w[4] || g->b[4]};
    bool below[7];   // below[k]: something at a stage < k is asked for
    below[0] = false;
    for (int k = 0; k < 6; ++k) below[k + 1] = below[k] || want[k];
    if (!below[6]) return CID_OK;

    // fc
    const long long F = (long long)dm.features(), P4 = (long long)dm.ho[3] * dm.wo[3];
    if (want[5]) {
        const EsdFcBwdArgs fa{a[3], grad_logit, g->w[4], g->b[4], F, P4, (long long)N};
        hipLaunchKernelGGL(k_esd_fc_bwd, dim3((unsigned)((F + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, s, fa);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("fc");
    }
    if (!below[5]) return CID_OK;

    const auto wg_args = [&](int i, const EsdDzSrc& dz, const float* ain) {
        const int l = i + 1;
        return EsdWgradArgs{dz, ain, part, part_b, (long long)N * q.wg_tiles[i], q.wg_splits[i], kEsdConv[l].cout, dm.ho[l - 1], dm.wo[l - 1],
                            dm.ho[l], dm.wo[l], q.wg_tiles_x[i], q.wg_tiles[i]};
    };
    const auto dg_args = [&](int i, const EsdDzSrc& dz, float* out) {
        const int l = i + 1;
        return EsdDgradArgs{dz, blob + d->blob.off[l], out, dm.ho[l - 1], dm.wo[l - 1], dm.ho[l], dm.wo[l], q.dg_tiles_x[i], 0};
    };

    // conv4: the gradient of a4 is dl[n] * fc.weight, formed in staging
    const EsdDzSrc dz4{a[3], nullptr, grad_logit, blob + d->blob.fcw, (size_t)F};
    if (want[4] && esd_wgrad_launch<kEsdWgCD[2], 256, true>(wg_args(2, dz4, a[2]), g->w[3], g->b[3], s) != hipSuccess) return cx.hip("wgrad4");
    if (!below[4]) return CID_OK;
    if (esd_dgrad_launch<512, 256, kEsdDgCXW[2], kEsdDgPT[2], true>(dg_args(2, dz4, da[2]), q.dg_tiles[2], N, s) != hipSuccess)
        return cx.hip("dgrad4");
    // conv3
    const EsdDzSrc dz3{a[2], da[2], nullptr, nullptr, 0};
    if (want[3] && esd_wgrad_launch<kEsdWgCD[1], 128, false>(wg_args(1, dz3, a[1]), g->w[2], g->b[2], s) != hipSuccess) return cx.hip("wgrad3");
    if (!below[3]) return CID_OK;
    if (esd_dgrad_launch<256, 128, kEsdDgCXW[1], kEsdDgPT[1], false>(dg_args(1, dz3, da[1]), q.dg_tiles[1], N, s) != hipSuccess)
        return cx.hip("dgrad3");
    // conv2
    const EsdDzSrc dz2{a[1], da[1], nullptr, nullptr, 0};
    if (want[2] && esd_wgrad_launch<kEsdWgCD[0], 64, false>(wg_args(0, dz2, a[0]), g->w[1], g->b[1], s) != hipSuccess) return cx.hip("wgrad2");
    if (!below[2]) return CID_OK;
    if (esd_dgrad_launch<128, 64, kEsdDgCXW[0], kEsdDgPT[0], false>(dg_args(0, dz2, da[0]), q.dg_tiles[0], N, s) != hipSuccess)
        return cx.hip("dgrad2");
    // conv1
    if (want[1]) {
        const EsdWgrad1Args wa{in, a[0], da[0], part1, (long long)N * q.w1_strips, q.w1_splits, q.w1_strips, H, W, dm.ho[0], dm.wo[0]};
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esd_wgrad1<true>, dim3((unsigned)q.w1_splits), dim3(D_THREADS), 0, s, wa);
        else hipLaunchKernelGGL(k_esd_wgrad1<false>, dim3((unsigned)q.w1_splits), dim3(D_THREADS), 0, s, wa);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("wgrad1");
        const DiscWgrad0ReduceArgs r{part1, g->w[0], g->b[0], q.w1_splits};
        hipLaunchKernelGGL(k_disc_wgrad0_reduce, dim3((64 * 28 + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, s, r);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("wgrad1 reduce");
    }
    if (want[0]) {
        const int hc = cdiv(H, 2), wc = cdiv(W, 2);
        if (const int rc = cx.launches(N, "dgrad1", [&](int n0, int n) {
            const EsdDgrad1Args ga{a[0], da[0], blob + d->blob.off[0], g->input, H, W, dm.ho[0], dm.wo[0], n0};
            const dim3 grid((unsigned)(((long long)hc * wc + D_THREADS - 1) / D_THREADS), (unsigned)n, 4);
            hipLaunchKernelGGL(k_esd_dgrad1, grid, dim3(D_THREADS), 0, s, ga);
        })) return rc;
    }
    return CID_OK;
}

int cid_esd_pack_weights_device(cid_esd_t d, const float* const* dev_params, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const std::string fn = "cid_esd_pack_weights_device: ";
    if (!dev_params || !device_blob) return d->fail(CID_ERR_INVALID, fn + "null pointer");
    for (int i = 0; i < CID_ESD_NUM_WEIGHTS; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3)) return d->fail(CID_ERR_INVALID, fn + "null or misaligned parameter pointer");
    if ((uintptr_t)device_blob & 255) return d->fail(CID_ERR_WORKSPACE, fn + "blob must be 256-byte aligned");
    static_assert(CID_ESD_NUM_WEIGHTS == 2 * (kEsdConvs + 1), "a weight and a bias per layer");
    EsdPackArgs a{};
    for (int i = 0; i <= kEsdConvs; ++i) {
        a.w[i] = dev_params[2 * i];
        a.b[i] = dev_params[2 * i + 1];
    }
    for (int i = 0; i < kEsdConvs; ++i) a.off[i] = (long long)d->blob.off[i];
    a.blob = static_cast<float*>(device_blob);
    a.fcw = (long long)d->blob.fcw;
    a.fcb = (long long)d->blob.fcb;
    a.total = (long long)d->blob.total;
    const EsdDims dims(d->H, d->W);
    a.P = (long long)dims.ho[3] * dims.wo[3];
    hipLaunchKernelGGL(k_esd_pack, dim3((unsigned)((a.total + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return d->fail(CID_ERR_HIP, fn + "launch failed");
    d->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

}  // extern "C"
