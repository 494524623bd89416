// The BatchNorm discriminators (cid_disc_*, cid_srd_*) described once: a table per family (DiscNet), and over it the blob layout, the
// forward's and the saved forward's plans, the handle with its weight staging, the argument checks and the forward's launch sequence
// (disc_forward: the trunk model.0 ... model.10, which the families share, around the family's own top).  Then the denoise trainer's
// discriminator itself: its table, its head and its entry points.  Kernels in disc_kernels.h.  Host code.
#pragma once
#include "../api_common.h"
#include "../disc_kernels.h"

#include <cmath>
#include <cstring>
#include <initializer_list>
#include <vector>

namespace {

constexpr int kDiscMaxConvs = 7;
// part: output channels per packed block of an MFMA layer (pack_mfma_layer); 0: the layer keeps the reference layout
struct DiscConvDef { const char* name; int cin, cout, k, stride, part; };

// One family.  conv[0 ... 3] and bn_c[0 ... 2] are the trunk (model.0, 2, 5, 8 and BatchNorms 3, 6, 9), the same in every table: the
// kernels' template arguments fix them.  MFMA layer l = conv[l + 1], followed by BatchNorm l.
struct DiscNet {
    const char* prefix;     // the family's name in every message: "cid_disc", "cid_srd"
    const char* bn_names;   // its BatchNorms, as the unknown-key message names them
    int nconv;
    DiscConvDef conv[kDiscMaxConvs];
    int nbn, bn_c[D_MAX_BNS], maxc;   // the BatchNorms' channels and the widest
    int head_keep[2];       // doubles per image a saved forward keeps of the head: pooled means, hidden pre-activations
    // Blob segments (floats, each 64-float aligned): weights then biases of each convolution, in the reference layout or packed.
    size_t off[kDiscMaxConvs], total;

    constexpr DiscNet(const char* family, const char* bns, std::initializer_list<DiscConvDef> convs, std::initializer_list<int> bn_channels,
                      int pooled, int hidden)
        : prefix(family), bn_names(bns), nconv(0), conv{}, nbn(0), bn_c{}, maxc(0), head_keep{pooled, hidden}, off{}, total(0) {
        for (const DiscConvDef& L : convs) {
            off[nconv] = total;
            total = align64(total + (size_t)L.cout * L.cin * L.k * L.k + L.cout);
            conv[nconv++] = L;
        }
        for (const int c : bn_channels) {
            bn_c[nbn++] = c;
            maxc = c > maxc ? c : maxc;
        }
    }
};

struct DiscPlan {
    int H, W, H2, W2, H4, W4;
    int tiles_x[D_MAX_BNS], tiles[D_MAX_BNS];   // MFMA layers: conv launches 2, 5, 8 (and 11)
    size_t regA, regB, st, slab[D_MAX_BNS], total;
    // output and input size of MFMA layer l
    int ho(int l) const { return l < 2 ? H2 : H4; }
    int wo(int l) const { return l < 2 ? W2 : W4; }
    int hin(int l) const { return l ? ho(l - 1) : H; }
    int win(int l) const { return l ? wo(l - 1) : W; }
    long long pix(int l) const { return (long long)ho(l) * wo(l); }
};

// Output rows per tile of the MFMA layers; the last is model.11 of the SRGAN discriminator, which runs in 128-channel halves.
constexpr int kDiscTileRows[D_MAX_BNS] = {DiscGeom<64, 64, 2>::TH, DiscGeom<64, 128, 1>::TH, DiscGeom<128, 128, 2>::TH,
                                          DiscGeom<128, 128, 1>::TH};

int disc_plan(const DiscNet& net, int N, int H, int W, int training, DiscPlan& p) {
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;   // the layer-0 kernel indexes an image's pixels with int
    p.H = H;
    p.W = W;
    p.H2 = (H - 1) / 2 + 1;
    p.W2 = (W - 1) / 2 + 1;
    p.H4 = (p.H2 - 1) / 2 + 1;
    p.W4 = (p.W2 - 1) / 2 + 1;
    if (training && (long long)N * p.H4 * p.W4 == 1) return CID_ERR_SHAPE;
    const size_t n = (size_t)N, f = sizeof(float);
    // The layers' outputs alternate between two regions.  A: a0 (64 x H x W), later z5 (128 x H2 x W2), later z11 (256 x H4 x W4,
    // where the family has it); B: z2 (64 x H2 x W2), later z8 (128 x H4 x W4)
    size_t reg[2] = {n * net.conv[0].cout * H * W, 0};
    for (int l = 0; l < net.nbn; ++l) {
        p.tiles_x[l] = (p.wo(l) + D_TW - 1) / D_TW;
        p.tiles[l] = ((p.ho(l) + kDiscTileRows[l] - 1) / kDiscTileRows[l]) * p.tiles_x[l];
        size_t& r = reg[(l + 1) & 1];
        r = std::max(r, n * net.conv[l + 1].cout * p.ho(l) * p.wo(l));
    }
    size_t at = 0;
    p.regA = take(at, reg[0] * f);
    p.regB = take(at, reg[1] * f);
    p.st = take(at, (size_t)net.nbn * net.maxc * 2 * f);
    for (int l = 0; l < net.nbn; ++l) {
        p.slab[l] = at;
        if (training) at += align256((size_t)net.bn_c[l] * 2 * n * p.tiles[l] * sizeof(double));
    }
    p.total = at;
    return CID_OK;
}

// What cid_*_forward_saved keeps for one call.
struct DiscSavedPlan {
    size_t z[D_MAX_BNS + 1], st, mi, pooled, hidden, slab[D_MAX_BNS], total;
};

void disc_saved_plan(const DiscNet& net, int N, int training, const DiscPlan& p, DiscSavedPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    size_t at = 0;
    q.z[0] = take(at, n * net.conv[0].cout * p.H * p.W * f);
    for (int l = 0; l < net.nbn; ++l) q.z[l + 1] = take(at, n * net.conv[l + 1].cout * p.ho(l) * p.wo(l) * f);
    q.st = take(at, (size_t)net.nbn * net.maxc * 2 * f);
    q.mi = take(at, (size_t)net.nbn * net.maxc * 2 * sizeof(double));
    q.pooled = take(at, n * net.head_keep[0] * sizeof(double));
    q.hidden = take(at, n * net.head_keep[1] * sizeof(double));
    for (int l = 0; l < net.nbn; ++l) q.slab[l] = training ? take(at, (size_t)net.bn_c[l] * 2 * n * p.tiles[l] * sizeof(double)) : at;
    q.total = at;
}

// Where one forward keeps its tensors: two overlapping workspace regions (cid_*_forward) or a per-call buffer (cid_*_forward_saved).
struct DiscBufs {
    float* z[D_MAX_BNS + 1];     // the activated a0, then the raw z2, z5, z8 (and z11)
    float* st[D_MAX_BNS];        // (scale, shift) pairs of the BatchNorms
    double* mi[D_MAX_BNS];       // (mean, invstd) pairs, or null
    double* slab[D_MAX_BNS];     // train mode: per-tile partial sums
    double *pooled, *hidden;     // what a saved forward keeps of the head (DiscNet::head_keep), or null
};

DiscBufs disc_workspace_bufs(const DiscNet& net, void* workspace, const DiscPlan& p) {
    char* ws = static_cast<char*>(workspace);
    DiscBufs b{};
    for (int l = 0; l <= net.nbn; ++l) b.z[l] = reinterpret_cast<float*>(ws + (l & 1 ? p.regB : p.regA));
    for (int l = 0; l < net.nbn; ++l) {
        b.st[l] = reinterpret_cast<float*>(ws + p.st) + l * net.maxc * 2;
        b.slab[l] = reinterpret_cast<double*>(ws + p.slab[l]);
    }
    return b;
}

DiscBufs disc_saved_bufs(const DiscNet& net, void* saved, const DiscSavedPlan& q) {
    char* sv = static_cast<char*>(saved);
    DiscBufs b{};
    for (int l = 0; l <= net.nbn; ++l) b.z[l] = reinterpret_cast<float*>(sv + q.z[l]);
    for (int l = 0; l < net.nbn; ++l) {
        b.st[l] = reinterpret_cast<float*>(sv + q.st) + l * net.maxc * 2;
        b.mi[l] = reinterpret_cast<double*>(sv + q.mi) + l * net.maxc * 2;
        b.slab[l] = reinterpret_cast<double*>(sv + q.slab[l]);
    }
    b.pooled = reinterpret_cast<double*>(sv + q.pooled);
    b.hidden = reinterpret_cast<double*>(sv + q.hidden);
    return b;
}

// The handle of a family: its table and the host copy of the blob as cid_*_set_weight stages it.
struct DiscHandle : HandleBase {
    const DiscNet& net;
    std::vector<float> staging;
    bool have[kDiscMaxConvs][2] = {};
    explicit DiscHandle(const DiscNet& n) : net(n), staging(n.total, 0.f) {}
};

template <class Handle>
int disc_create(Handle** out) {
    if (!out) return CID_ERR_INVALID;
    *out = new (std::nothrow) Handle();
    return *out ? CID_OK : CID_ERR_INVALID;
}

// cid_*_set_weight
int disc_set_weight(DiscHandle* d, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!d) return CID_ERR_INVALID;
    const DiscNet& net = d->net;
    const std::string fn = std::string(net.prefix) + "_set_weight: ";
    if (!key || !data || (!shape && ndim > 0)) return d->fail(CID_ERR_INVALID, fn + "null argument");
    const std::string k(key);
    int li = -1, is_bias = 0;
    for (int i = 0; i < net.nconv; ++i) {
        if (k == std::string(net.conv[i].name) + ".weight") { li = i; is_bias = 0; }
        if (k == std::string(net.conv[i].name) + ".bias") { li = i; is_bias = 1; }
    }
    if (li < 0)
        return d->fail(CID_ERR_KEY, fn + "unknown key '" + k + "' (BatchNorm tensors " + net.bn_names + " are passed to " + net.prefix +
                                        "_forward, not staged)");
    const auto& L = net.conv[li];
    const int64_t want_w[4] = {L.cout, L.cin, L.k, L.k};
    const bool ok = is_bias ? (ndim == 1 && shape[0] == L.cout)
                            : (ndim == 4 && std::equal(shape, shape + 4, want_w));
    if (!ok) return d->fail(CID_ERR_SHAPE, fn + "size mismatch for " + k);
    float* seg = d->staging.data() + net.off[li];
    const size_t nw = (size_t)L.cout * L.cin * L.k * L.k;
    if (L.part) pack_mfma_layer(seg, is_bias ? nullptr : data, is_bias ? data : nullptr, L.cin, L.cout, L.part);
    else std::memcpy(is_bias ? seg + nw : seg, data, (is_bias ? (size_t)L.cout : nw) * sizeof(float));
    d->have[li][is_bias] = true;
    return CID_OK;
}

// cid_*_upload_weights
int disc_upload_weights(DiscHandle* d, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const std::string fn = std::string(d->net.prefix) + "_upload_weights: ";
    if (!device_blob) return d->fail(CID_ERR_INVALID, fn + "null device pointer");
    if ((uintptr_t)device_blob & 255) return d->fail(CID_ERR_WORKSPACE, fn + "blob must be 256-byte aligned");
    for (int i = 0; i < d->net.nconv; ++i)
        if (!d->have[i][0] || !d->have[i][1]) return d->fail(CID_ERR_STATE, fn + d->net.conv[i].name + " not set");
    return d->upload_blob(fn, device_blob, d->staging.data(), d->staging.size(), stream);
}

// cid_*_workspace_bytes
int disc_workspace_bytes(const DiscNet& net, int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    return plan_bytes(disc_plan(net, N, H, W, training, p), p, bytes);
}

// One MFMA convolution layer over a plan's tiles.  COUT_TOTAL > COUT: the layer's COUT-channel parts are the grid's z (k_disc_conv).
template <int CIN, int COUT, int S, bool BN_IN, int COUT_TOTAL = COUT>
hipError_t disc_conv_launch(const DiscConvArgs& base, int layer, const DiscPlan& p, int N, bool training, hipStream_t s) {
    (void)for_each_launch(N, [&](int n0, int n) {
        DiscConvArgs a = base;
        a.n0 = n0;
        a.tiles_x = p.tiles_x[layer];
        a.tiles = p.tiles[layer];
        const dim3 grid((unsigned)p.tiles[layer], (unsigned)n, COUT_TOTAL / COUT), block(D_THREADS);
        if (training) hipLaunchKernelGGL((k_disc_conv<CIN, COUT, S, BN_IN, true, COUT_TOTAL>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_disc_conv<CIN, COUT, S, BN_IN, false, COUT_TOTAL>), grid, block, 0, s, a);
    });
    return hipGetLastError();
}

bool disc_finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

// The checks of bn[0 .. count - 1] every entry point that takes cid_disc_bn shares; momentum and the counter count in train mode.
int disc_check_bn(const Call& cx, const cid_disc_bn* bn, int count, int training) {
    for (int l = 0; l < count; ++l) {
        const cid_disc_bn& b = bn[l];
        if (!b.gamma || !b.beta || !b.running_mean || !b.running_var || (training && !b.num_batches_tracked))
            return cx.fail(CID_ERR_INVALID, "null BatchNorm pointer");
        if (!disc_finite_nonneg(b.eps)) return cx.fail(CID_ERR_INVALID, "eps must be finite and >= 0");
        if (training && !(disc_finite_nonneg(b.momentum) || b.momentum == CID_DISC_MOMENTUM_NONE))
            return cx.fail(CID_ERR_INVALID, "momentum must be finite and >= 0, or CID_DISC_MOMENTUM_NONE");
    }
    return CID_OK;
}

// The argument checks every forward entry point of the discriminators shares, in the order cid.h documents, then the plan; `buf` is
// its workspace or saved buffer.
int disc_check_forward(const Call& cx, const DiscNet& net, const void* in, int in_fmt, const float* out, int N, int H, int W,
                       const cid_disc_bn* bn, int training, const void* buf, DiscPlan& p) {
    if (!in || !out || !bn || !buf) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) return cx.fail(CID_ERR_INVALID, "unknown input format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || ((uintptr_t)out & 3))
        return cx.fail(CID_ERR_INVALID, "misaligned fp32 operand");
    if (training != 0 && training != 1) return cx.fail(CID_ERR_INVALID, "training must be 0 or 1");
    if (const int rc = disc_check_bn(cx, bn, net.nbn, training)) return rc;
    if (disc_plan(net, N, H, W, training, p) != CID_OK)
        return training && N >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL
                   ? cx.h->fail(CID_ERR_SHAPE, "Expected more than 1 value per channel when training")
                   : cx.fail(CID_ERR_SHAPE, "input shape not accepted (N, H, W >= 1, H*W < 2^31)");
    return CID_OK;
}

// Train-mode statistics of one C-channel BatchNorm from its layer's slab: (scale, shift) into `st`, the running buffers updated.
hipError_t disc_stats_launch(const cid_disc_bn& bn, int C, const double* slab, long long rows, double count, float* st, double* mi,
                             hipStream_t s) {
    DiscStatsArgs a{};
    a.slab = slab;
    a.rows = rows;
    a.count = count;
    a.gamma = bn.gamma;
    a.beta = bn.beta;
    a.running_mean = bn.running_mean;
    a.running_var = bn.running_var;
    a.num_batches_tracked = reinterpret_cast<const long long*>(bn.num_batches_tracked);
    a.eps = bn.eps;
    a.momentum = bn.momentum == CID_DISC_MOMENTUM_NONE ? -1.0 : bn.momentum;
    a.st = st;
    a.mi = mi;
    hipLaunchKernelGGL(k_disc_bn_stats, dim3(C), dim3(D_THREADS), 0, s, a);
    return hipPeekAtLastError();
}

// One forward on checked arguments: what the trunk and a family's top launch from.
struct DiscFwd {
    const Call& cx;
    const DiscNet& net;
    const cid_disc_bn* bn;
    int N, training;
    DiscPlan p;
    DiscBufs b;

    const float* w(int conv) const { return cx.h->dev_blob + net.off[conv]; }   // a convolution's segment of the blob

    // The tensors of MFMA layer l's launch: from z[l] (through BatchNorm l - 1 + LeakyReLU where l > 0) to z[l + 1].
    DiscConvArgs conv_args(int l) const {
        DiscConvArgs a{};
        a.in = b.z[l];
        a.out = b.z[l + 1];
        a.w = w(l + 1);
        a.st_in = l ? b.st[l - 1] : nullptr;
        a.slab = training ? b.slab[l] : nullptr;
        a.rows = (long long)N * p.tiles[l];
        a.Hin = p.hin(l);
        a.Win = p.win(l);
        a.Ho = p.ho(l);
        a.Wo = p.wo(l);
        return a;
    }

    // Train-mode statistics of BatchNorm l from its layer's slab.
    hipError_t stats(int l) const {
        return disc_stats_launch(bn[l], net.bn_c[l], b.slab[l], (long long)N * p.tiles[l], (double)N * (double)p.pix(l), b.st[l], b.mi[l], cx.s);
    }
};

// The forward's launch sequence: the eval-mode BatchNorms, the trunk, then top(f, out), the family's layers above BatchNorm 9 down to
// the probabilities, then the BatchNorm counters.
template <class Top>
int disc_forward_run(const DiscFwd& f, const void* in, int in_fmt, float* out, Top&& top) {
    const Call& cx = f.cx;
    const DiscNet& net = f.net;
    const DiscPlan& p = f.p;
    const int N = f.N;
    const bool training = f.training;
    const hipStream_t s = cx.s;

    if (!training) {
        DiscBnEvalArgs e{};
        for (int l = 0; l < net.nbn; ++l) {
            e.gamma[l] = f.bn[l].gamma;
            e.beta[l] = f.bn[l].beta;
            e.running_mean[l] = f.bn[l].running_mean;
            e.running_var[l] = f.bn[l].running_var;
            e.eps[l] = f.bn[l].eps;
            e.st[l] = f.b.st[l];
            e.C[l] = net.bn_c[l];
            e.mi[l] = f.b.mi[l];
        }
        hipLaunchKernelGGL(k_disc_bn_eval, dim3(net.nbn), dim3(D_BN_MAXC), 0, s, e);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn_eval");
    }
    // layer 0 (model.0 + LeakyReLU -> a0)
    if (const int rc = cx.launches(N, "conv0", [&](int n0, int n) {
        DiscConv0Args a{in, f.b.z[0], f.w(0), p.H, p.W, n0};
        const dim3 grid((unsigned)(((long long)p.H * p.W + D_THREADS - 1) / D_THREADS), (unsigned)n);
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_disc_conv0<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_disc_conv0<false>, grid, dim3(D_THREADS), 0, s, a);
    })) return rc;
    // layer 2 (reads a0, writes z2), BN3
    if (disc_conv_launch<64, 64, 2, false>(f.conv_args(0), 0, p, N, training, s) != hipSuccess) return cx.hip("conv2");
    if (training && f.stats(0) != hipSuccess) return cx.hip("bn3 stats");
    // layer 5 (reads z2 through BN3 + LeakyReLU, writes z5), BN6
    if (disc_conv_launch<64, 128, 1, true>(f.conv_args(1), 1, p, N, training, s) != hipSuccess) return cx.hip("conv5");
    if (training && f.stats(1) != hipSuccess) return cx.hip("bn6 stats");
    // layer 8 (reads z5 through BN6 + LeakyReLU, writes z8), BN9
    if (disc_conv_launch<128, 128, 2, true>(f.conv_args(2), 2, p, N, training, s) != hipSuccess) return cx.hip("conv8");
    if (training && f.stats(2) != hipSuccess) return cx.hip("bn9 stats");
    if (const int rc = top(f, out)) return rc;
    if (training) {
        DiscBnCountArgs c{};
        for (int l = 0; l < net.nbn; ++l) c.count[l] = reinterpret_cast<long long*>(f.bn[l].num_batches_tracked);
        c.n = net.nbn;
        hipLaunchKernelGGL(k_disc_bn_count, dim3(1), dim3(64), 0, s, c);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("bn count");
    }
    return CID_OK;
}

// cid_*_forward (`saved` false: `buf` is the workspace) and cid_*_forward_saved (`buf` is the call's saved buffer), entry point `fn`.
template <class Top>
int disc_forward(DiscHandle* d, const char* fn, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn,
                 int training, void* buf, size_t buf_bytes, bool saved, void* stream, Top&& top) {
    if (!d) return CID_ERR_INVALID;
    const DiscNet& net = d->net;
    const Call cx(d, fn, stream);
    DiscFwd f{cx, net, bn, N, training, {}, {}};
    if (const int rc = disc_check_forward(cx, net, in, in_fmt, out, N, H, W, bn, training, buf, f.p)) return rc;
    if (saved) {
        DiscSavedPlan q;
        disc_saved_plan(net, N, training, f.p, q);
        if (const int rc = cx.room(buf, buf_bytes, q.total, (std::string(net.prefix) + "_saved_bytes").c_str(), "saved buffer")) return rc;
        f.b = disc_saved_bufs(net, buf, q);
    } else {
        if (const int rc = cx.room(buf, buf_bytes, f.p.total, (std::string(net.prefix) + "_workspace_bytes").c_str())) return rc;
        f.b = disc_workspace_bufs(net, buf, f.p);
    }
    if (const int rc = cx.uploaded()) return rc;
    return disc_forward_run(f, in, in_fmt, out, top);
}

// ---------------------------------------------------------------------------------------------------------------------------
// The denoise trainer's discriminator.
constexpr DiscNet kDiscNet("cid_disc", "model.3/6/9",
                           {{"model.0", 3, 64, 3, 1, 0}, {"model.2", 64, 64, 3, 2, 64}, {"model.5", 64, 128, 3, 1, 128},
                            {"model.8", 128, 128, 3, 2, 128}, {"model.12", 128, 1, 1, 1, 0}},
                           {64, 128, 128}, 0, 0);

// Its top: BN9 + LeakyReLU, average pool, 1x1 conv, sigmoid.
int disc_head_launches(const DiscFwd& f, float* out) {
    return f.cx.launches(f.N, "head", [&](int n0, int n) {
        DiscHeadArgs a{f.b.z[3], f.b.st[2], f.w(4), out, f.p.pix(2), n0};
        hipLaunchKernelGGL(k_disc_head, dim3((unsigned)n), dim3(D_HEAD_THREADS), 0, f.cx.s, a);
    });
}

}  // namespace

struct cid_disc_s : DiscHandle {
    cid_disc_s() : DiscHandle(kDiscNet) {}
};

extern "C" {

int cid_disc_create(cid_disc_t* out) { return disc_create(out); }

void cid_disc_destroy(cid_disc_t d) { delete d; }

const char* cid_disc_last_error(cid_disc_t d) { return d ? d->err.c_str() : "null handle"; }

int cid_disc_set_weight(cid_disc_t d, const char* key, const float* data, const int64_t* shape, int ndim) {
    return disc_set_weight(d, key, data, shape, ndim);
}

size_t cid_disc_packed_weights_bytes(void) { return kDiscNet.total * sizeof(float); }

int cid_disc_upload_weights(cid_disc_t d, void* device_blob, void* stream) { return disc_upload_weights(d, device_blob, stream); }

int cid_disc_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    return disc_workspace_bytes(kDiscNet, N, H, W, training, bytes);
}

int cid_disc_forward(cid_disc_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn,
                     int training, void* workspace, size_t workspace_bytes, void* stream) {
    return disc_forward(d, "cid_disc_forward", in, in_fmt, out, N, H, W, bn, training, workspace, workspace_bytes, false, stream,
                        disc_head_launches);
}

}  // extern "C"
