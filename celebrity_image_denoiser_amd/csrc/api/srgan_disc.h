// The SRGAN trainer's discriminator (cid_srd_*): its table, its top and its entry points.  Layers model.0 ... model.10 are the denoise
// discriminator's trunk and everything about weights, plans and the launch sequence is the shared description's (disc_forward.h);
// model.11 runs on k_disc_conv as two 128-channel halves; the head is in srgan_disc_kernels.h.  Host code.
#pragma once
#include "disc_forward.h"
#include "../srgan_disc_kernels.h"

namespace {

constexpr int kSrdHalf = 128;   // channels per workgroup of model.11: k_disc_conv<128, 128, 1, ., ., 256>

// model.0, model.15 and model.17 keep the reference layout; model.11 is packed as two blocks, one per half: [16][9][8][128] of output
// channels 128*half ... 128*half + 127, then their 128 biases.
constexpr DiscNet kSrdNet("cid_srd", "model.3/6/9/12",
                          {{"model.0", 3, 64, 3, 1, 0}, {"model.2", 64, 64, 3, 2, 64}, {"model.5", 64, 128, 3, 1, 128},
                           {"model.8", 128, 128, 3, 2, 128}, {"model.11", 128, 256, 3, 1, kSrdHalf}, {"model.15", 256, 512, 1, 1, 0},
                           {"model.17", 512, 1, 1, 1, 0}},
                          {64, 128, 128, 256}, SRD_HEAD_C, SRD_HEAD_HID);

// Its top: layer 11 (reads z8 through BN9 + LeakyReLU, writes z11 in two 128-channel halves), BN12, then the head: BN12 + LeakyReLU,
// average pool, the two 1x1 convolutions, sigmoid.  A saved forward's head also keeps its pooled means and hidden pre-activations.
int srd_top_launches(const DiscFwd& f, float* out) {
    const Call& cx = f.cx;
    if (disc_conv_launch<128, kSrdHalf, 1, true, 256>(f.conv_args(3), 3, f.p, f.N, f.training, cx.s) != hipSuccess) return cx.hip("conv11");
    if (f.training && f.stats(3) != hipSuccess) return cx.hip("bn12 stats");
    return cx.launches(f.N, "head", [&](int n0, int n) {
        SrdHeadArgs a{f.b.z[4], f.b.st[3], f.w(5), f.w(6), out, f.p.pix(3), n0};
        if (f.b.pooled) {
            SrdHeadSavedArgs as{a, f.b.pooled, f.b.hidden};
            hipLaunchKernelGGL(k_srd_head_saved, dim3((unsigned)n), dim3(SRD_HEAD_THREADS), 0, cx.s, as);
        } else {
            hipLaunchKernelGGL(k_srd_head, dim3((unsigned)n), dim3(SRD_HEAD_THREADS), 0, cx.s, a);
        }
    });
}

}  // namespace

struct cid_srd_s : DiscHandle {
    cid_srd_s() : DiscHandle(kSrdNet) {}
};

extern "C" {

int cid_srd_create(cid_srd_t* out) { return disc_create(out); }

void cid_srd_destroy(cid_srd_t d) { delete d; }

const char* cid_srd_last_error(cid_srd_t d) { return d ? d->err.c_str() : "null handle"; }

int cid_srd_set_weight(cid_srd_t d, const char* key, const float* data, const int64_t* shape, int ndim) {
    return disc_set_weight(d, key, data, shape, ndim);
}

size_t cid_srd_packed_weights_bytes(void) { return kSrdNet.total * sizeof(float); }

int cid_srd_upload_weights(cid_srd_t d, void* device_blob, void* stream) { return disc_upload_weights(d, device_blob, stream); }

int cid_srd_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    return disc_workspace_bytes(kSrdNet, N, H, W, training, bytes);
}

int cid_srd_forward(cid_srd_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn, int training,
                    void* workspace, size_t workspace_bytes, void* stream) {
    return disc_forward(d, "cid_srd_forward", in, in_fmt, out, N, H, W, bn, training, workspace, workspace_bytes, false, stream,
                        srd_top_launches);
}

int cid_srd_losses(const float* p_real, const float* p_fake, int N, double* out, void* stream) {
    if (!p_real || !p_fake || !out) return CID_ERR_INVALID;
    if (((uintptr_t)p_real & 3) || ((uintptr_t)p_fake & 3) || ((uintptr_t)out & 7)) return CID_ERR_INVALID;
    if (N < 1) return CID_ERR_SHAPE;
    SrdLossArgs a{p_real, p_fake, N, out};
    hipLaunchKernelGGL(k_srd_losses, dim3(1), dim3(D_LOSS_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"
