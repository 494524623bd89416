// The BatchNorm discriminators' backward side, shared over the family tables of disc_forward.h: the backward's tiling, the stages from
// BatchNorm 9 down to the input (disc_bwd_lower), its checks, the device pack and the masks.  Then the denoise discriminator's own:
// its backward plan and head, and the entry points of its saved forward, backward pass, device pack, masks and losses (cid_disc_*).
// Kernels in disc_bwd_kernels.h.  Host code.
#pragma once
#include "../disc_bwd_kernels.h"
#include "disc_forward.h"

namespace {

// How the launches of layers 2, 5, 8 and 0 tile one backward call, and what the scratch regions they share must hold
// (disc_bwd_tiling); then where a family's backward plan puts those regions in its workspace.
struct DiscBwdTiling {
    int strips[3];                  // BatchNorm strips per image
    int wg_tiles_x[3], wg_tiles[3]; // wgrad items per image of layers 2, 5, 8
    int wg_splits[3];
    int dg_tiles_x[3], dg_tiles[3]; // dgrad tiles of the largest class
    int w0_strips, w0_splits;
    size_t max_bnslab, max_part, max_part_b;   // bytes, the largest of the three layers
    // X holds the gradient of a6 and later of a0, Y the gradient of a3 (the forward's two regions); coef has maxc * D_COEF floats per
    // BatchNorm
    size_t coef, bnslab, X, Y, part, part_b, part0;
};

constexpr int kDiscWgCD[3] = {64, 128, 128}, kDiscWgCX[3] = {64, 64, 128}, kDiscWgS[3] = {2, 1, 2};
constexpr int kDiscDgTileRows[3] = {DiscDgradGeom<64, 64, 2>::TH, DiscDgradGeom<128, 64, 1>::TH, DiscDgradGeom<128, 128, 2>::TH};

void disc_bwd_tiling(const DiscNet& net, int N, const DiscPlan& p, DiscBwdTiling& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    const int H = p.H, W = p.W;
    const int ho[3] = {p.H2, p.H2, p.H4}, wo[3] = {p.W2, p.W2, p.W4};
    const int hin[3] = {H, p.H2, p.H2}, win[3] = {W, p.W2, p.W2};
    q.max_bnslab = q.max_part = q.max_part_b = 0;
    for (int l = 0; l < 3; ++l) {
        q.strips[l] = (int)(((long long)ho[l] * wo[l] + D_BN_STRIP - 1) / D_BN_STRIP);
        q.max_bnslab = std::max(q.max_bnslab, (size_t)net.bn_c[l] * 2 * n * q.strips[l] * sizeof(double));
        q.wg_tiles_x[l] = (wo[l] + D_TW - 1) / D_TW;
        q.wg_tiles[l] = ((ho[l] + D_WG_TH - 1) / D_WG_TH) * q.wg_tiles_x[l];
        const long long items = (long long)N * q.wg_tiles[l];
        q.wg_splits[l] = (int)std::min<long long>(items, 512 / (kDiscWgCX[l] / 16));
        q.max_part = std::max(q.max_part, (size_t)q.wg_splits[l] * kDiscWgCX[l] * kDiscWgCD[l] * 9 * f);
        q.max_part_b = std::max(q.max_part_b, (size_t)q.wg_splits[l] * kDiscWgCD[l] * sizeof(double));
        const int hc = (hin[l] + kDiscWgS[l] - 1) / kDiscWgS[l], wc = (win[l] + kDiscWgS[l] - 1) / kDiscWgS[l];
        q.dg_tiles_x[l] = (wc + D_TW - 1) / D_TW;
        q.dg_tiles[l] = ((hc + kDiscDgTileRows[l] - 1) / kDiscDgTileRows[l]) * q.dg_tiles_x[l];
    }
    q.w0_strips = (int)(((long long)H * W + 63) / 64);
    q.w0_splits = (int)std::min<long long>((long long)N * q.w0_strips, 1024);
}

// The trailing template arguments are the kernels' (disc_bwd_kernels.h); at their defaults the launches are the denoise discriminator's.
template <int CD, int CX, int S, bool BN_IN, bool HEAD, bool POOL = false, int CD_TOTAL = CD>
hipError_t disc_wgrad_launch(const DiscWgradArgs& a, float* dw, float* db, hipStream_t s) {
    hipLaunchKernelGGL((k_disc_wgrad<CD, CX, S, BN_IN, HEAD, POOL, CD_TOTAL>), dim3((unsigned)a.splits, CX / 16, CD_TOTAL / CD), dim3(D_THREADS),
                       0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const DiscWgradReduceArgs r{a.part, a.part_b, dw, db, a.splits, CD_TOTAL, CX};
    hipLaunchKernelGGL(k_disc_wgrad_reduce, dim3((CD_TOTAL * CX * 9 + CD_TOTAL + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, s, r);
    return hipGetLastError();
}

template <int CD, int CX, int S, bool HEAD, bool POOL = false, int CD_PART = CD>
hipError_t disc_dgrad_launch(const DiscDgradArgs& base, int tiles, int N, hipStream_t s) {
    (void)for_each_launch(N, [&](int n0, int n) {
        DiscDgradArgs a = base;
        a.n0 = n0;
        const dim3 grid((unsigned)tiles, (unsigned)n, DiscDgradGeom<CD, CX, S>::CLASSES);
        hipLaunchKernelGGL((k_disc_dgrad<CD, CX, S, HEAD, POOL, CD_PART>), grid, dim3(D_THREADS), 0, s, a);
    });
    return hipGetLastError();
}

template <int C, bool HEAD, bool POOL = false>
hipError_t disc_bn_part_launch(const DiscBnPartArgs& base, int N, hipStream_t s) {
    (void)for_each_launch(N, [&](int n0, int n) {
        DiscBnPartArgs a = base;
        a.n0 = n0;
        hipLaunchKernelGGL((k_disc_bn_bwd_part<C, HEAD, POOL>), dim3((unsigned)a.strips, (unsigned)n), dim3(D_THREADS), 0, s, a);
    });
    return hipGetLastError();
}

// The arguments of one launch, as both discriminators' backward passes build them.
hipError_t disc_bn_reduce_launch(int C, const double* bnslab, long long rows, double count, const cid_disc_bn& bn, const float* st,
                                 const double* mi, int training, float* coef, float* dgamma, float* dbeta, hipStream_t s) {
    DiscBnRedArgs a{bnslab, rows, count, bn.gamma, st, mi, training, coef, dgamma, dbeta};
    hipLaunchKernelGGL(k_disc_bn_bwd_reduce, dim3(C), dim3(D_THREADS), 0, s, a);
    return hipPeekAtLastError();
}

DiscBnPartArgs disc_bn_part_args(const float* z, const float* up, const float* dl, const float* coef, const float* st, const double* mi,
                                 double* bnslab, int N, int strips, long long pix) {
    return DiscBnPartArgs{z, up, dl, coef, st, mi, bnslab, (long long)N * strips, pix, strips, 0};
}

DiscWgradArgs disc_wgrad_args(const DiscDzSrc& dz, const float* ain, const float* st_in, float* part, double* part_b, int N, int tiles_x,
                              int tiles, int splits, int Hin, int Win, int Ho, int Wo) {
    DiscWgradArgs a{};
    a.dz = dz;
    a.ain = ain;
    a.st_in = st_in;
    a.part = part;
    a.part_b = part_b;
    a.items = (long long)N * tiles;
    a.splits = splits;
    a.Hin = Hin;
    a.Win = Win;
    a.Ho = Ho;
    a.Wo = Wo;
    a.tiles_x = tiles_x;
    a.tiles = tiles;
    return a;
}

DiscDgradArgs disc_dgrad_args(const DiscDzSrc& dz, const float* w, float* out, int tiles_x, int Hin, int Win, int Ho, int Wo) {
    DiscDgradArgs a{};
    a.dz = dz;
    a.w = w;
    a.out = out;
    a.Hin = Hin;
    a.Win = Win;
    a.Ho = Ho;
    a.Wo = Wo;
    a.tiles_x = tiles_x;
    return a;
}

// The stages both discriminators share, BatchNorm 9 down to the input, on one call's tensors.
struct DiscBwdLower {
    const void* in;
    int in_fmt, N, H, W, H2, W2, H4, W4, training;
    const cid_disc_bn* bn;             // BatchNorms 3, 6, 9
    const int* bn_c;                   // their channels
    const float *a0, *z2, *z5, *z8;    // saved by the forward
    float* const* st;                  // [3]
    double* const* mi;                 // [3]
    const float* w[4];                 // model.0, 2, 5, 8 in the packed blob
    float *gw[4], *gb[4], *ggamma[3], *gbeta[3], *ginput;   // what is asked for (null: not)
    float* coef[3];                    // scratch, where the family's plan put it (DiscBwdTiling)
    double* bnslab;
    float *X, *Y, *part;
    double *part_b, *part0;
    // something at or below BatchNorm 9 is asked for
    bool wanted() const {
        bool any = ginput != nullptr;
        for (int i = 0; i < 4; ++i) any = any || gw[i] || gb[i];
        for (int l = 0; l < 3; ++l) any = any || ggamma[l] || gbeta[l];
        return any;
    }
};

// BatchNorm 9's upstream gradient is the head's rank-one form (HEAD: dl[N] and coef[2]'s slot 7, the denoise discriminator) or the
// tensor up9 (the SRGAN discriminator: the data gradient of its model.11, which may be Y).
template <bool HEAD>
int disc_bwd_lower(const Call& cx, const DiscBwdLower& c, const DiscBwdTiling& q, const float* up9, const float* dl) {
    const hipStream_t s = cx.s;
    const int N = c.N, H = c.H, W = c.W;
    // what is asked for at each stage: bn9(7) > conv8(6) > bn6(5) > conv5(4) > bn3(3) > conv2(2) > conv0(1) > input(0)
    const bool want[8] = {c.ginput != nullptr, c.gw[0] || c.gb[0], c.gw[1] || c.gb[1], c.ggamma[0] || c.gbeta[0], c.gw[2] || c.gb[2],
                          c.ggamma[1] || c.gbeta[1], c.gw[3] || c.gb[3], c.ggamma[2] || c.gbeta[2]};
    bool below[9];   // below[k]: something at a stage < k is asked for
    below[0] = false;
    for (int k = 0; k < 8; ++k) below[k + 1] = below[k] || want[k];
    if (!below[8]) return CID_OK;
    const long long P4 = (long long)c.H4 * c.W4, P2 = (long long)c.H2 * c.W2;

    const auto bn_reduce = [&](int l, long long pix) {
        return disc_bn_reduce_launch(c.bn_c[l], c.bnslab, (long long)N * q.strips[l], (double)N * (double)pix, c.bn[l], c.st[l], c.mi[l],
                                     c.training, c.coef[l], c.ggamma[l], c.gbeta[l], s);
    };
    const auto bn_part = [&](int l, const float* z, const float* up, long long pix) {
        return disc_bn_part_args(z, up, dl, c.coef[l], c.st[l], c.mi[l], c.bnslab, N, q.strips[l], pix);
    };
    const auto wg_args = [&](int l, const DiscDzSrc& dz, const float* ain, const float* st_in, int Hin, int Win, int Ho, int Wo) {
        return disc_wgrad_args(dz, ain, st_in, c.part, c.part_b, N, q.wg_tiles_x[l], q.wg_tiles[l], q.wg_splits[l], Hin, Win, Ho, Wo);
    };
    const auto dg_args = [&](int l, int ci, const DiscDzSrc& dz, float* out, int Hin, int Win, int Ho, int Wo) {
        return disc_dgrad_args(dz, c.w[ci], out, q.dg_tiles_x[l], Hin, Win, Ho, Wo);
    };
    float* const X = c.X;
    float* const Y = c.Y;

    // BN9, layer 8
    if (disc_bn_part_launch<128, HEAD>(bn_part(2, c.z8, up9, P4), N, s) != hipSuccess) return cx.hip("bn9 sums");
    if (bn_reduce(2, P4) != hipSuccess) return cx.hip("bn9 reduce");
    const DiscDzSrc dz8{c.z8, up9, dl, c.coef[2]};
    if (want[6] && disc_wgrad_launch<128, 128, 2, true, HEAD>(wg_args(2, dz8, c.z5, c.st[1], c.H2, c.W2, c.H4, c.W4), c.gw[3], c.gb[3], s) != hipSuccess)
        return cx.hip("wgrad8");
    if (!below[6]) return CID_OK;
    if (disc_dgrad_launch<128, 128, 2, HEAD>(dg_args(2, 3, dz8, X, c.H2, c.W2, c.H4, c.W4), q.dg_tiles[2], N, s) != hipSuccess) return cx.hip("dgrad8");
    // BN6, layer 5
    if (disc_bn_part_launch<128, false>(bn_part(1, c.z5, X, P2), N, s) != hipSuccess) return cx.hip("bn6 sums");
    if (bn_reduce(1, P2) != hipSuccess) return cx.hip("bn6 reduce");
    const DiscDzSrc dz5{c.z5, X, nullptr, c.coef[1]};
    if (want[4] && disc_wgrad_launch<128, 64, 1, true, false>(wg_args(1, dz5, c.z2, c.st[0], c.H2, c.W2, c.H2, c.W2), c.gw[2], c.gb[2], s) != hipSuccess)
        return cx.hip("wgrad5");
    if (!below[4]) return CID_OK;
    if (disc_dgrad_launch<128, 64, 1, false>(dg_args(1, 2, dz5, Y, c.H2, c.W2, c.H2, c.W2), q.dg_tiles[1], N, s) != hipSuccess) return cx.hip("dgrad5");
    // BN3, layer 2
    if (disc_bn_part_launch<64, false>(bn_part(0, c.z2, Y, P2), N, s) != hipSuccess) return cx.hip("bn3 sums");
    if (bn_reduce(0, P2) != hipSuccess) return cx.hip("bn3 reduce");
    const DiscDzSrc dz2{c.z2, Y, nullptr, c.coef[0]};
    if (want[2] && disc_wgrad_launch<64, 64, 2, false, false>(wg_args(0, dz2, c.a0, nullptr, H, W, c.H2, c.W2), c.gw[1], c.gb[1], s) != hipSuccess)
        return cx.hip("wgrad2");
    if (!below[2]) return CID_OK;
    if (disc_dgrad_launch<64, 64, 2, false>(dg_args(0, 1, dz2, X, H, W, c.H2, c.W2), q.dg_tiles[0], N, s) != hipSuccess) return cx.hip("dgrad2");
    // layer 0
    if (want[1]) {
        DiscWgrad0Args a{c.in, c.a0, X, c.part0, (long long)N * q.w0_strips, q.w0_splits, q.w0_strips, H, W};
        if (c.in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_disc_wgrad0<true>, dim3((unsigned)q.w0_splits), dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_disc_wgrad0<false>, dim3((unsigned)q.w0_splits), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("wgrad0");
        DiscWgrad0ReduceArgs r{c.part0, c.gw[0], c.gb[0], q.w0_splits};
        hipLaunchKernelGGL(k_disc_wgrad0_reduce, dim3((64 * 28 + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, s, r);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("wgrad0 reduce");
    }
    if (want[0]) {
        if (const int rc = cx.launches(N, "dgrad0", [&](int n0, int n) {
            DiscDgrad0Args a{c.a0, X, c.w[0], c.ginput, H, W, n0};
            const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), (unsigned)n);
            hipLaunchKernelGGL(k_disc_dgrad0, grid, dim3(D_THREADS), 0, s, a);
        })) return rc;
    }
    return CID_OK;
}

// A family's gradient struct (cid_disc_grads, cid_srd_grads) as pointers; all null where the caller passed none.
struct DiscGrads {
    float* const* w;
    float* const* b;
    float* const* gamma;
    float* const* beta;
    float* input;
};

template <class G>
DiscGrads disc_grads(const G* g) { return g ? DiscGrads{g->w, g->b, g->gamma, g->beta, g->input} : DiscGrads{}; }

// What a backward entry point does before its own plan: the argument and shape checks in the order cid.h documents (`grads` is the
// caller's struct, g its pointers) and the saved buffer's size; p gets the forward's plan and sv the saved tensors.
int disc_bwd_prepare(const Call& cx, const DiscNet& net, const void* in, int in_fmt, const float* grad_prob, int N, int H, int W,
                     const cid_disc_bn* bn, int training, const void* saved, size_t saved_bytes, const void* grads, const DiscGrads& g,
                     const void* workspace, DiscPlan& p, DiscBufs& sv) {
    if (!in || !grad_prob || !bn || !saved || !grads || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) return cx.fail(CID_ERR_INVALID, "unknown input format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || ((uintptr_t)grad_prob & 3))
        return cx.fail(CID_ERR_INVALID, "misaligned fp32 operand");
    for (int l = 0; l < net.nbn; ++l)
        if (!bn[l].gamma) return cx.fail(CID_ERR_INVALID, "null BatchNorm weight pointer");
    bool misaligned = ((uintptr_t)g.input & 3) != 0;
    for (int i = 0; i < net.nconv; ++i) misaligned = misaligned || ((uintptr_t)g.w[i] & 3) || ((uintptr_t)g.b[i] & 3);
    for (int l = 0; l < net.nbn; ++l) misaligned = misaligned || ((uintptr_t)g.gamma[l] & 3) || ((uintptr_t)g.beta[l] & 3);
    if (misaligned) return cx.fail(CID_ERR_INVALID, "misaligned gradient pointer");
    if (g.input && in_fmt != CID_FMT_F32_NCHW)
        return cx.fail(CID_ERR_INVALID, "a uint8 input has no gradient (grads.input must be null)");
    if (training != 0 && training != 1) return cx.fail(CID_ERR_INVALID, "training must be 0 or 1");
    if (disc_plan(net, N, H, W, training, p) != CID_OK)
        return cx.fail(CID_ERR_SHAPE, "shape not accepted (N, H, W >= 1, H*W < 2^31, more than one value per channel in train mode)");
    DiscSavedPlan sp;
    disc_saved_plan(net, N, training, p, sp);
    if (const int rc = cx.room(saved, saved_bytes, sp.total, (std::string(net.prefix) + "_saved_bytes").c_str(), "saved buffer")) return rc;
    sv = disc_saved_bufs(net, const_cast<void*>(saved), sp);
    return CID_OK;
}

// The shared stages' tensors of one backward call: the saved forward `sv` (which must outlive the result), the gradients asked for
// and the scratch regions of the family's plan q in `workspace`.
DiscBwdLower disc_bwd_lower_args(const Call& cx, const DiscNet& net, const void* in, int in_fmt, int N, const DiscPlan& p, int training,
                                 const cid_disc_bn* bn, const DiscBufs& sv, const DiscGrads& g, void* workspace, const DiscBwdTiling& q) {
    char* ws = static_cast<char*>(workspace);
    DiscBwdLower c{};
    c.in = in;
    c.in_fmt = in_fmt;
    c.N = N, c.H = p.H, c.W = p.W, c.H2 = p.H2, c.W2 = p.W2, c.H4 = p.H4, c.W4 = p.W4;
    c.training = training;
    c.bn = bn;
    c.bn_c = net.bn_c;
    c.a0 = sv.z[0], c.z2 = sv.z[1], c.z5 = sv.z[2], c.z8 = sv.z[3];
    c.st = sv.st;
    c.mi = sv.mi;
    for (int i = 0; i < 4; ++i) {
        c.w[i] = cx.h->dev_blob + net.off[i];
        c.gw[i] = g.w[i];
        c.gb[i] = g.b[i];
    }
    for (int l = 0; l < 3; ++l) {
        c.ggamma[l] = g.gamma[l];
        c.gbeta[l] = g.beta[l];
        c.coef[l] = reinterpret_cast<float*>(ws + q.coef) + l * net.maxc * D_COEF;
    }
    c.ginput = g.input;
    c.bnslab = reinterpret_cast<double*>(ws + q.bnslab);
    c.X = reinterpret_cast<float*>(ws + q.X);
    c.Y = reinterpret_cast<float*>(ws + q.Y);
    c.part = reinterpret_cast<float*>(ws + q.part);
    c.part_b = reinterpret_cast<double*>(ws + q.part_b);
    c.part0 = reinterpret_cast<double*>(ws + q.part0);
    return c;
}

// cid_*_saved_bytes
int disc_saved_bytes(const DiscNet& net, int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    DiscSavedPlan q;
    const int rc = disc_plan(net, N, H, W, training, p);
    if (rc == CID_OK) disc_saved_plan(net, N, training, p, q);
    return plan_bytes(rc, q, bytes);
}

// cid_*_pack_weights_device: the blob of cid_*_set_weight + cid_*_upload_weights from the 2 * nconv parameter tensors on the device.
int disc_pack_weights_device(DiscHandle* d, const float* const* dev_params, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const DiscNet& net = d->net;
    const std::string fn = std::string(net.prefix) + "_pack_weights_device: ";
    if (!dev_params || !device_blob) return d->fail(CID_ERR_INVALID, fn + "null pointer");
    for (int i = 0; i < 2 * net.nconv; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3)) return d->fail(CID_ERR_INVALID, fn + "null or misaligned parameter pointer");
    if ((uintptr_t)device_blob & 255) return d->fail(CID_ERR_WORKSPACE, fn + "blob must be 256-byte aligned");
    static_assert(kDiscMaxConvs == D_PACK_LAYERS, "one slot per convolution");
    DiscPackArgs a{};
    for (int i = 0; i < net.nconv; ++i) {
        const auto& L = net.conv[i];
        a.w[i] = dev_params[2 * i];
        a.b[i] = dev_params[2 * i + 1];
        a.off[i] = (int)net.off[i];
        a.cin[i] = L.cin;
        a.cout[i] = L.cout;
        a.kk[i] = L.k * L.k;
        a.part[i] = L.part;
    }
    a.blob = static_cast<float*>(device_blob);
    a.layers = net.nconv;
    a.total = (int)net.total;
    hipLaunchKernelGGL(k_disc_pack, dim3((a.total + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return d->fail(CID_ERR_HIP, fn + "launch failed");
    d->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

// cid_*_saved_masks: the masks of a0 and of every BatchNorm's output, masks[0 ... nbn]; the caller's array has `nmasks` entries.  sv
// gets the saved tensors, for a family with a further mask of its own.
int disc_saved_masks(const DiscNet& net, const void* saved, size_t saved_bytes, int N, int H, int W, int training,
                     unsigned char* const* masks, int nmasks, void* stream, DiscBufs& sv) {
    if (!saved || !masks || (training != 0 && training != 1)) return CID_ERR_INVALID;
    for (int i = 0; i < nmasks; ++i)
        if (!masks[i]) return CID_ERR_INVALID;
    DiscPlan p;
    const int rc = disc_plan(net, N, H, W, training, p);
    if (rc != CID_OK) return rc;
    DiscSavedPlan sp;
    disc_saved_plan(net, N, training, p, sp);
    if (saved_bytes < sp.total || ((uintptr_t)saved & 255)) return CID_ERR_WORKSPACE;
    sv = disc_saved_bufs(net, const_cast<void*>(saved), sp);
    for (int i = 0; i <= net.nbn; ++i) {
        const int C = net.conv[i].cout;
        const long long P = i ? p.pix(i - 1) : (long long)H * W;
        DiscMaskArgs a{sv.z[i], i ? sv.st[i - 1] : nullptr, masks[i], (long long)N * C * P, P, C};
        const long long blocks = (a.total + D_THREADS - 1) / D_THREADS;
        if (blocks > 0x7fffffffLL) return CID_ERR_SHAPE;
        hipLaunchKernelGGL(k_disc_masks, dim3((unsigned)blocks), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
        if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
    }
    return CID_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// Workspace of the denoise discriminator's backward call.
struct DiscBwdPlan : DiscBwdTiling {
    size_t dl, mean, total;
};

void disc_bwd_plan(int N, const DiscPlan& p, DiscBwdPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    const int H = p.H, W = p.W;
    disc_bwd_tiling(kDiscNet, N, p, q);
    size_t at = 0;
    q.dl = take(at, n * f);
    q.mean = take(at, n * 128 * sizeof(double));
    q.coef = take(at, 3 * 128 * D_COEF * f);
    q.bnslab = take(at, q.max_bnslab);
    q.X = take(at, std::max(n * 128 * p.H2 * p.W2, n * 64 * H * W) * f);
    q.Y = take(at, n * 64 * p.H2 * p.W2 * f);
    q.part = take(at, q.max_part);
    q.part_b = take(at, q.max_part_b);
    q.part0 = take(at, (size_t)q.w0_splits * 64 * 28 * sizeof(double));
    q.total = at;
}

}  // namespace

extern "C" {

int cid_disc_saved_bytes(int N, int H, int W, int training, size_t* bytes) { return disc_saved_bytes(kDiscNet, N, H, W, training, bytes); }

int cid_disc_forward_saved(cid_disc_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn,
                           int training, void* saved, size_t saved_bytes, void* stream) {
    return disc_forward(d, "cid_disc_forward_saved", in, in_fmt, out, N, H, W, bn, training, saved, saved_bytes, true, stream,
                        disc_head_launches);
}

int cid_disc_backward_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    DiscBwdPlan q;
    const int rc = disc_plan(kDiscNet, N, H, W, training, p);
    if (rc == CID_OK) disc_bwd_plan(N, p, q);
    return plan_bytes(rc, q, bytes);
}

int cid_disc_backward(cid_disc_t d, const void* in, int in_fmt, const float* grad_prob, int N, int H, int W, const cid_disc_bn* bn,
                      int training, const void* saved, size_t saved_bytes, const cid_disc_grads* grads, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const Call cx(d, "cid_disc_backward", stream);
    const DiscGrads g = disc_grads(grads);
    DiscPlan p;
    DiscBufs sv;
    if (const int rc = disc_bwd_prepare(cx, kDiscNet, in, in_fmt, grad_prob, N, H, W, bn, training, saved, saved_bytes, grads, g, workspace, p, sv))
        return rc;
    DiscBwdPlan q;
    disc_bwd_plan(N, p, q);
    if (const int rc = cx.room(workspace, workspace_bytes, q.total, "cid_disc_backward_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;

    const hipStream_t s = cx.s;
    char* ws = static_cast<char*>(workspace);
    float* dl = reinterpret_cast<float*>(ws + q.dl);
    double* mean = reinterpret_cast<double*>(ws + q.mean);
    const float* w12 = d->dev_blob + kDiscNet.off[4];
    const DiscBwdLower c = disc_bwd_lower_args(cx, kDiscNet, in, in_fmt, N, p, training, bn, sv, g, workspace, q);
    if (!(c.wanted() || g.w[4] || g.b[4])) return CID_OK;
    const long long P4 = (long long)p.H4 * p.W4;

    // head (stage 8); the rest is the shared chain, with BatchNorm 9's upstream dl[n] * w12[c] / P4
    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        DiscHeadBwdArgs a{sv.z[3], sv.st[2], w12, grad_prob, mean, dl, P4, n0};
        hipLaunchKernelGGL(k_disc_head_bwd, dim3((unsigned)n), dim3(D_HEAD_THREADS), 0, s, a);
    })) return rc;
    {
        DiscHeadReduceArgs a{mean, dl, w12, g.w[4], g.b[4], c.coef[2], (double)P4, N};
        hipLaunchKernelGGL(k_disc_head_reduce, dim3(1), dim3(128), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("head reduce");
    }
    return disc_bwd_lower<true>(cx, c, q, nullptr, dl);
}

int cid_disc_pack_weights_device(cid_disc_t d, const float* const* dev_params, void* device_blob, void* stream) {
    static_assert(CID_DISC_NUM_WEIGHTS == 2 * kDiscNet.nconv, "a weight and a bias per convolution");
    return disc_pack_weights_device(d, dev_params, device_blob, stream);
}

int cid_disc_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int training, unsigned char* const* masks, void* stream) {
    DiscBufs sv;
    return disc_saved_masks(kDiscNet, saved, saved_bytes, N, H, W, training, masks, kDiscNet.nbn + 1, stream, sv);
}

int cid_disc_losses(const float* p_real, const float* p_fake, const void* den, int d_fmt, const void* clean, int c_fmt,
                    int N, int H, int W, double* out, void* stream) {
    if (!p_real || !p_fake || !den || !clean || !out) return CID_ERR_INVALID;
    if (!fmt_ok(den, d_fmt) || !fmt_ok(clean, c_fmt) || ((uintptr_t)p_real & 3) || ((uintptr_t)p_fake & 3) || ((uintptr_t)out & 7))
        return CID_ERR_INVALID;
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    DiscLossArgs a{p_real, p_fake, den, clean, d_fmt, c_fmt, N, (long long)H * W, out};
    hipLaunchKernelGGL(k_disc_losses, dim3(1), dim3(D_LOSS_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
