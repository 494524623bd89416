// The ESRGAN generator in train mode (cid_esr_forward_train): workspace plan, argument checks and launch sequence.  Head and tail are
// cid_esr_forward's launches (esrgan.h); the trunk runs on esrgan_train_kernels.h with the statistics kernel and the cid_disc_bn
// contract of the discriminators (disc_forward.h).  The run takes a struct of buffer pointers, as sr_train_run does (srgan_train.h), so
// that cid_esr_forward_saved (esrgan_backward.h) can point the same launches into its saved buffer.  Host code.
#pragma once
#include "../esrgan_train_kernels.h"
#include "disc_forward.h"
#include "esrgan.h"

namespace {

static_assert(2 * kEsrMaxBlocks <= E_TRAIN_MAX_BNS, "k_esr_bn_count holds every BatchNorm's counter");

struct EsrTrainPlan {
    // byte offsets: x1, the two raw z tensors the 2 R convolutions alternate between, the two tensors the blocks' outputs alternate
    // between (the tail's input takes the one the last block's input is not in), the slab every convolution reuses (64 channels x 2
    // sums x N * ctiles rows of fp64), the 2 R (scale, shift) tables, each on its own 256-byte boundary
    size_t x1, z[2], r[2], slab, st[2 * kEsrMaxBlocks], total;
    int ctiles_x, ctiles, ttiles_x, ttiles;
    int tail_r;   // which of r[] the tail reads
};

int esr_train_plan(int N, int H, int W, int R, EsrTrainPlan& p) {
    if (R < 0 || R > kEsrMaxBlocks) return CID_ERR_INVALID;
    EsrPlan e;
    if (const int rc = esr_plan(N, H, W, e)) return rc;
    if (R > 0 && (long long)N * H * W == 1) return CID_ERR_SHAPE;   // one value per channel has no variance
    p.ctiles_x = e.ctiles_x;
    p.ctiles = e.ctiles;
    p.ttiles_x = e.ttiles_x;
    p.ttiles = e.ttiles;
    p.tail_r = R ? (R - 1) % 2 : 0;
    const size_t t = (size_t)N * 64 * H * W * sizeof(float);
    size_t at = 0;
    p.x1 = take(at, t);
    p.z[0] = take(at, t);
    p.z[1] = take(at, t);
    p.r[0] = take(at, t);
    p.r[1] = take(at, t);
    p.slab = take(at, (size_t)64 * 2 * N * p.ctiles * sizeof(double));
    for (int l = 0; l < 2 * R; ++l) p.st[l] = take(at, (size_t)64 * 2 * sizeof(float));
    p.total = at;
    return CID_OK;
}

// Where one train-mode forward writes.  cid_esr_forward_train points everything into its workspace, where the z and the block outputs
// each alternate between two tensors; block i's output r[i] (i < R - 1) must not share a tensor with r[i - 1] or x1, nor tail_in with
// the last block's input.
struct EsrTrainBufs {
    float* x1;
    float* z[2 * kEsrMaxBlocks];
    float* r[kEsrMaxBlocks];
    float* tail_in;
    double* slab;
    float* st[2 * kEsrMaxBlocks];    // one (scale, shift) table per BatchNorm
    double* mi[2 * kEsrMaxBlocks];   // one (mean, invstd) table per BatchNorm, or null
    float* v0;                       // the head's sums before PReLU (cid_esr_forward_saved), or null
};

EsrTrainBufs esr_train_bufs(void* workspace, int R, const EsrTrainPlan& p) {
    char* ws = static_cast<char*>(workspace);
    EsrTrainBufs b{};
    b.x1 = reinterpret_cast<float*>(ws + p.x1);
    for (int l = 0; l < 2 * R; ++l) {
        b.z[l] = reinterpret_cast<float*>(ws + p.z[l % 2]);
        b.st[l] = reinterpret_cast<float*>(ws + p.st[l]);
    }
    for (int i = 0; i + 1 < R; ++i) b.r[i] = reinterpret_cast<float*>(ws + p.r[i % 2]);
    b.tail_in = reinterpret_cast<float*>(ws + p.r[p.tail_r]);
    b.slab = reinterpret_cast<double*>(ws + p.slab);
    return b;
}

// The message of a shape esr_train_plan refused.
int esr_train_shape_fail(const Call& cx, int N, int H, int W) {
    if (N < 1 || H < 1 || W < 1 || (long long)N * H * W != 1) return cx.fail(CID_ERR_SHAPE, "input shape not accepted (N, H, W >= 1, H*W < 2^31)");
    return cx.h->fail(CID_ERR_SHAPE, "Expected more than 1 value per channel when training");
}

int esr_train_check(const Call& cx, cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W,
                    const cid_disc_bn* bn, const void* workspace, EsrTrainPlan& p) {
    if (const int rc = check_image_io(cx, in, in_fmt, out, out_fmt, workspace)) return rc;
    if (h->R > 0) {   // with no block there is no BatchNorm to describe
        if (!bn) return cx.fail(CID_ERR_INVALID, "null pointer");
        if (const int rc = disc_check_bn(cx, bn, 2 * h->R, 1)) return rc;
    }
    return esr_train_plan(N, H, W, h->R, p) == CID_OK ? CID_OK : esr_train_shape_fail(cx, N, H, W);
}

int esr_train_run(const Call& cx, cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W,
                  const cid_disc_bn* bn, const EsrTrainPlan& p, const EsrTrainBufs& b);

}  // namespace

extern "C" {

int cid_esr_train_workspace_bytes(int N, int H, int W, int num_residuals, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    EsrTrainPlan p;
    return plan_bytes(esr_train_plan(N, H, W, num_residuals, p), p, bytes);
}

int cid_esr_train_stage_view(const char* stage, int N, int H, int W, int num_residuals, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                             int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    EsrTrainPlan p;
    if (const int rc = esr_train_plan(N, H, W, num_residuals, p)) return rc;
    const std::string s(stage);
    if (s == "x1") *offset_bytes = p.x1;
    else if (s == "tail_in") *offset_bytes = p.r[p.tail_r];
    else return CID_ERR_KEY;
    *C = 64;
    *Hs = H;
    *Ws = W;
    *channel_block = 8;
    return CID_OK;
}

int cid_esr_forward_train(cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, const cid_disc_bn* bn,
                          void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_esr_forward_train", stream);
    EsrTrainPlan p;
    if (const int rc = esr_train_check(cx, h, in, in_fmt, out, out_fmt, N, H, W, bn, workspace, p)) return rc;
    if (const int rc = cx.room(workspace, workspace_bytes, p.total, "cid_esr_train_workspace_bytes")) return rc;
    if (const int rc = cx.uploaded()) return rc;
    return esr_train_run(cx, h, in, in_fmt, out, out_fmt, N, H, W, bn, p, esr_train_bufs(workspace, h->R, p));
}

}  // extern "C"

namespace {

int esr_train_run(const Call& cx, cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W,
                  const cid_disc_bn* bn, const EsrTrainPlan& p, const EsrTrainBufs& b) {
    const hipStream_t s = cx.s;
    const float* blob = h->dev_blob;
    const int R = h->R, L = 2 * R;
    const long long rows = (long long)N * p.ctiles;

    // with no block the head writes the tail's input too (x1 + x1), as in cid_esr_forward
    if (const int rc = cx.launches(N, "head", [&](int n0, int n) {
        const EsrHeadArgs a{in, b.x1, R == 0 ? b.tail_in : nullptr, blob, H, W, n0};
        const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), (unsigned)n);
        if (b.v0) {
            const EsrHeadSavedArgs sa{a, b.v0};
            if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL((k_esr_head<true, true>), grid, dim3(D_THREADS), 0, s, sa);
            else hipLaunchKernelGGL((k_esr_head<false, true>), grid, dim3(D_THREADS), 0, s, sa);
        } else if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esr_head<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_esr_head<false>, grid, dim3(D_THREADS), 0, s, a);
    })) return rc;
    // launches 0 .. 2R-1: the blocks' convolutions, x1 -> z[0] -> z[1] -> ..., each followed by its BatchNorm's statistics.  An even
    // l > 0 is a block's first convolution: it forms the previous block's output r[l/2 - 1] from that block's input and BN(z[l - 1]).
    for (int l = 0; l < L; ++l) {
        if (const int rc = cx.launches(N, "trunk", [&](int n0, int n) {
            EsrTrainConvArgs a{};
            a.c.in = l == 0 ? b.x1 : b.z[l - 1];
            a.c.out = b.z[l];
            a.c.w = blob + kEsrHeadSeg + (size_t)l * kEsrConvSeg;
            a.c.st_in = l == 0 ? nullptr : b.st[l - 1];
            a.c.slope = l % 2 ? a.c.w - kEsrConvSeg + E_CONV_SLOPE : nullptr;   // the block's first convolution carries its slope
            a.c.slab = b.slab;
            a.c.rows = rows;
            a.c.H = H;
            a.c.W = W;
            a.c.tiles_x = p.ctiles_x;
            a.c.tiles = p.ctiles;
            a.c.n0 = n0;
            const dim3 grid((unsigned)p.ctiles, (unsigned)n), block(D_THREADS);
            if (l == 0) hipLaunchKernelGGL((k_sr_train_conv<ST_IN_RAW, ST_EPI_STATS>), grid, block, 0, s, a.c);
            else if (l % 2) hipLaunchKernelGGL((k_sr_train_conv<ST_IN_BN_PRELU, ST_EPI_STATS>), grid, block, 0, s, a.c);
            else {
                const int i = l / 2 - 1;   // the block whose output this launch forms
                a.res_in = i == 0 ? b.x1 : b.r[i - 1];
                a.r_out = b.r[i];
                hipLaunchKernelGGL(k_esr_train_conv, grid, block, 0, s, a);
            }
        })) return rc;
        if (disc_stats_launch(bn[l], 64, b.slab, rows, (double)N * (double)H * (double)W, b.st[l], b.mi[l], s) != hipSuccess)
            return cx.hip("bn stats");
    }
    if (R > 0) {
        EsrBnCountArgs c{};   // every statistics launch has read its counter
        for (int l = 0; l < L; ++l) c.count[l] = reinterpret_cast<long long*>(bn[l].num_batches_tracked);
        c.n = L;
        hipLaunchKernelGGL(k_esr_bn_count, dim3(1), dim3(64), 0, s, c);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn count");
        if (const int rc = cx.launches(N, "sum", [&](int n0, int n) {
            const EsrTrainSumArgs a{b.z[L - 1], R == 1 ? b.x1 : b.r[R - 2], b.x1, b.tail_in, b.st[L - 1], (long long)H * W, n0};
            const dim3 grid((unsigned)(((long long)H * W * 16 + D_THREADS - 1) / D_THREADS), (unsigned)n);
            hipLaunchKernelGGL(k_esr_train_sum, grid, dim3(D_THREADS), 0, s, a);
        })) return rc;
    }
    return cx.launches(N, "tail", [&](int n0, int n) {
        const EsrTailArgs a{b.tail_in, out, blob + kEsrHeadSeg + (size_t)L * kEsrConvSeg, H, W, p.ttiles_x, n0};
        const dim3 grid((unsigned)p.ttiles, (unsigned)n);
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esr_tail<true>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_esr_tail<false>, grid, dim3(E_TAIL_THREADS), 0, s, a);
    });
}

}  // namespace
