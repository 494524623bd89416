// The SRGAN generator in train mode (cid_sr_forward_train): workspace plan, argument checks and launch sequence.  Head, upscale stages
// and tail are cid_sr_forward's launches (srgan.h); the trunk runs on srgan_train_kernels.h with the statistics kernel and the
// cid_disc_bn contract of the discriminators (disc_forward.h).  The checks and the run are shared with cid_sr_forward_saved
// (srgan_backward.h), which points the same launches into its saved buffer.  Host code.
#pragma once
#include "../srgan_train_kernels.h"
#include "disc_forward.h"
#include "srgan.h"

namespace {

struct SrTrainPlan {
    int stages;
    // byte offsets: x0, the two raw z tensors the ten convolutions alternate between, mid's result, stage k's output, the slab every
    // convolution reuses (64 channels x 2 sums x N * ctiles rows of fp64), the ten (scale, shift) tables
    size_t x0, z[2], trunk, up[3], slab, st, total;
    int ctiles_x, ctiles;
};

int sr_train_plan(int N, int H, int W, int scale, SrTrainPlan& p) {
    SrPlan e;
    if (const int rc = sr_plan(N, H, W, scale, e)) return rc;
    if ((long long)N * H * W == 1) return CID_ERR_SHAPE;   // one value per channel has no variance
    p.stages = e.stages;
    p.ctiles_x = e.ctiles_x;
    p.ctiles = e.ctiles;
    const size_t t = (size_t)N * 64 * H * W * sizeof(float);
    size_t at = 0;
    p.x0 = take(at, t);
    p.z[0] = take(at, t);
    p.z[1] = take(at, t);
    p.trunk = take(at, t);
    for (int u = 0; u < p.stages; ++u) p.up[u] = take(at, t << (2 * (u + 1)));
    p.slab = take(at, (size_t)64 * 2 * N * p.ctiles * sizeof(double));
    p.st = take(at, (size_t)S_TRAIN_BNS * 64 * 2 * sizeof(float));
    p.total = at;
    return CID_OK;
}

// Where one train-mode forward writes.  cid_sr_forward_train points everything into its workspace and the ten z alternate between
// two tensors; cid_sr_forward_saved (srgan_backward.h) gives each z a tensor of its own in the saved buffer, asks for the
// (mean, invstd) tables and for the pre-activations of the head and the upscale stages.
struct SrTrainBufs {
    float* x0;
    float* z[S_TRAIN_BNS];
    float* trunk;
    float* up[3];
    double* slab;
    float* st;             // ten (scale, shift) tables
    double* mi;            // ten (mean, invstd) tables, or null
    float* pre0;           // the head's sums before PReLU, or null
    float* pre_up[3];      // with pre0: stage k's shuffled sums before PReLU
};

SrTrainBufs sr_train_bufs(void* workspace, const SrTrainPlan& p) {
    char* ws = static_cast<char*>(workspace);
    SrTrainBufs b{};
    b.x0 = reinterpret_cast<float*>(ws + p.x0);
    for (int l = 0; l < S_TRAIN_BNS; ++l) b.z[l] = reinterpret_cast<float*>(ws + p.z[l % 2]);
    b.trunk = reinterpret_cast<float*>(ws + p.trunk);
    for (int u = 0; u < p.stages; ++u) b.up[u] = reinterpret_cast<float*>(ws + p.up[u]);
    b.slab = reinterpret_cast<double*>(ws + p.slab);
    b.st = reinterpret_cast<float*>(ws + p.st);
    return b;
}

// The error of a shape sr_train_plan does not accept, in the words every train-mode entry point uses.
int sr_train_shape_fail(const Call& cx, int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1) return cx.fail(CID_ERR_SHAPE, "input shape not accepted (N, H, W >= 1)");
    return (long long)N * H * W == 1 ? cx.h->fail(CID_ERR_SHAPE, "Expected more than 1 value per channel when training")
                                     : cx.fail(CID_ERR_SHAPE, "input shape not accepted (scale^2 * H * W < 2^31)");
}

// The argument checks cid_sr_forward_train and cid_sr_forward_saved share, up to the plan.
int sr_train_check(const Call& cx, cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, unsigned flags,
                   const cid_disc_bn* bn, const void* workspace, SrTrainPlan& p) {
    if (const int rc = check_image_io(cx, in, in_fmt, out, out_fmt, workspace)) return rc;
    if (!bn) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (flags & ~(unsigned)CID_SR_RAW) return cx.fail(CID_ERR_INVALID, "unknown flags");
    if ((flags & CID_SR_RAW) && out_fmt != CID_FMT_F32_NCHW) return cx.fail(CID_ERR_INVALID, "CID_SR_RAW needs an fp32 output");
    if (const int rc = disc_check_bn(cx, bn, S_TRAIN_BNS, 1)) return rc;
    return sr_train_plan(N, H, W, h->scale, p) == CID_OK ? (int)CID_OK : sr_train_shape_fail(cx, N, H, W);
}

int sr_train_run(const Call& cx, cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, unsigned flags,
                 const cid_disc_bn* bn, const SrTrainPlan& p, const SrTrainBufs& b);

}  // namespace

extern "C" {

int cid_sr_train_workspace_bytes(int N, int H, int W, int scale_factor, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    SrTrainPlan p;
    return plan_bytes(sr_train_plan(N, H, W, scale_factor, p), p, bytes);
}

int cid_sr_train_stage_view(const char* stage, int N, int H, int W, int scale_factor, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                            int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    SrTrainPlan p;
    if (const int rc = sr_train_plan(N, H, W, scale_factor, p)) return rc;
    const std::string s(stage);
    int shift = 0;
    if (s == "x0") *offset_bytes = p.x0;
    else if (s == "trunk") *offset_bytes = p.trunk;
    else if (s == "up1" && p.stages >= 2) *offset_bytes = p.up[0], shift = 1;
    else if (s == "up2" && p.stages >= 3) *offset_bytes = p.up[1], shift = 2;
    else if (s == "tail_in") *offset_bytes = p.stages ? p.up[p.stages - 1] : p.trunk, shift = p.stages;
    else return CID_ERR_KEY;
    *C = 64;
    *Hs = H << shift;
    *Ws = W << shift;
    *channel_block = 8;
    return CID_OK;
}

int cid_sr_forward_train(cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, unsigned flags,
                         const cid_disc_bn* bn, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_sr_forward_train", stream);
    SrTrainPlan p;
    if (const int rc = sr_train_check(cx, h, in, in_fmt, out, out_fmt, N, H, W, flags, bn, workspace, p)) return rc;
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_sr_train_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    return sr_train_run(cx, h, in, in_fmt, out, out_fmt, N, H, W, flags, bn, p, sr_train_bufs(workspace, p));
}

}  // extern "C"

namespace {

int sr_train_run(const Call& cx, cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, unsigned flags,
                 const cid_disc_bn* bn, const SrTrainPlan& p, const SrTrainBufs& b) {
    const hipStream_t s = cx.s;
    float* x0 = b.x0;
    float* trunk = b.trunk;
    double* slab = b.slab;
    float* st = b.st;
    const float* blob = h->dev_blob;
    const long long rows = (long long)N * p.ctiles;

    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        const SrHeadArgs a{in, x0, blob, H, W, H, W, 0, 0, n0};
        const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), (unsigned)n);
        const SrHeadSavedArgs as{a, b.pre0};
        if (b.pre0 && in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL((k_sr_head<true, true>), grid, dim3(D_THREADS), 0, s, as);
        else if (b.pre0) hipLaunchKernelGGL((k_sr_head<false, true>), grid, dim3(D_THREADS), 0, s, as);
        else if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_sr_head<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_sr_head<false>, grid, dim3(D_THREADS), 0, s, a);
    })) return rc;
    // launches 0 .. 9: the blocks' convolutions, x0 -> z[0] -> z[1] -> ..., each followed by its BatchNorm's statistics;
    // launch 10: mid(BN_9(z[9])) + x0 -> trunk
    for (int l = 0; l <= S_TRAIN_BNS; ++l) {
        if (l == S_TRAIN_BNS) {   // every statistics launch has read its counter
            SrBnCountArgs c{};
            for (int i = 0; i < S_TRAIN_BNS; ++i) c.count[i] = reinterpret_cast<long long*>(bn[i].num_batches_tracked);
            hipLaunchKernelGGL(k_sr_bn_count, dim3(1), dim3(64), 0, s, c);
            if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn count");
        }
        if (const int rc = cx.launches(N, "trunk", [&](int n0, int n) {
            SrTrainConvArgs a{};
            a.in = l == 0 ? x0 : b.z[l - 1];
            a.out = l == S_TRAIN_BNS ? trunk : b.z[l];
            a.res = x0;
            a.w = blob + kEsrHeadSeg + (size_t)l * kEsrConvSeg;
            a.st_in = l == 0 ? nullptr : st + (size_t)(l - 1) * 128;
            a.slope = l % 2 ? a.w - kEsrConvSeg + E_CONV_SLOPE : nullptr;   // the block's first convolution carries its slope
            a.slab = slab;
            a.rows = rows;
            a.H = H;
            a.W = W;
            a.tiles_x = p.ctiles_x;
            a.tiles = p.ctiles;
            a.n0 = n0;
            const dim3 grid((unsigned)p.ctiles, (unsigned)n), block(D_THREADS);
            if (l == S_TRAIN_BNS) hipLaunchKernelGGL((k_sr_train_conv<ST_IN_BN, ST_EPI_RES>), grid, block, 0, s, a);
            else if (l == 0) hipLaunchKernelGGL((k_sr_train_conv<ST_IN_RAW, ST_EPI_STATS>), grid, block, 0, s, a);
            else if (l % 2) hipLaunchKernelGGL((k_sr_train_conv<ST_IN_BN_PRELU, ST_EPI_STATS>), grid, block, 0, s, a);
            else hipLaunchKernelGGL((k_sr_train_conv<ST_IN_BN, ST_EPI_STATS>), grid, block, 0, s, a);
        })) return rc;
        if (l < S_TRAIN_BNS &&
            disc_stats_launch(bn[l], 64, slab, rows, (double)N * (double)H * (double)W, st + (size_t)l * 128,
                              b.mi ? b.mi + (size_t)l * 128 : nullptr, s) != hipSuccess)
            return cx.hip("bn stats");
    }
    // the upscale stages and the tail: cid_sr_forward's launches, which this call leaves as they are
    const float* u = trunk;
    int Hu = H, Wu = W;
    for (int k = 0; k < p.stages; ++k) {
        float* dst = b.up[k];
        const int tiles_x = (Wu + D_TW - 1) / D_TW;
        const int tiles = ((Hu + DiscGeom<64, 128, 1>::TH - 1) / DiscGeom<64, 128, 1>::TH) * tiles_x;
        if (const int rc = cx.launches(N, "upscale", [&](int n0, int n) {
            const SrUpArgs a{u, dst, blob + h->up_off(k), Hu, Wu, tiles_x, n0};
            const dim3 grid((unsigned)tiles, (unsigned)n, 2);
            const SrUpSavedArgs as{a, b.pre_up[k]};
            if (b.pre0) hipLaunchKernelGGL(k_sr_up<true>, grid, dim3(D_THREADS), 0, s, as);
            else hipLaunchKernelGGL(k_sr_up<>, grid, dim3(D_THREADS), 0, s, a);
        })) return rc;
        u = dst;
        Hu *= 2;
        Wu *= 2;
    }
    const int ttiles_x = (Wu + E_TAIL_TW - 1) / E_TAIL_TW;
    const int ttiles = ((Hu + E_TAIL_TH - 1) / E_TAIL_TH) * ttiles_x;
    return cx.launches(N, "tail", [&](int n0, int n) {
        const EsrTailArgs a{u, out, blob + h->tail_off(), Hu, Wu, ttiles_x, n0};
        const dim3 grid((unsigned)ttiles, (unsigned)n);
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_sr_tail<SR_OUT_U8>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else if (flags & CID_SR_RAW) hipLaunchKernelGGL(k_sr_tail<SR_OUT_RAW>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_sr_tail<SR_OUT_F32>, grid, dim3(E_TAIL_THREADS), 0, s, a);
    });
}

}  // namespace
