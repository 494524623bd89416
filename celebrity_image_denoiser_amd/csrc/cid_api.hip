// cid_api.hip — the C ABI of include/cid.h, one translation unit.  This file holds the denoising generator (cid_*: weight repacking,
// workspace planning, the launch sequence of one forward, the weight broadcast, the backward pass) and includes every other family's
// host file from api/; the device kernels are in the *_kernels.h headers, shared host plumbing in api_common.h and weight_store.h.
// Layer table = the reference module's declaration order, backend/app.py:42-78.
#include "../../include/cid.h"
#include "conv_kernels.h"
#include "wino64_kernels.h"
#include "wino42_kernels.h"
#include "conv_kernels_f16.h"
#include "quality_kernels.h"
#include "noise_kernels.h"
#include "disc_kernels.h"
#include "srgan_disc_kernels.h"
#include "esrgan_disc_kernels.h"
#include "disc_bwd_kernels.h"
#include "gen_bwd_kernels.h"
#include "gen_pack_kernels.h"
#include "optim_kernels.h"
#include "resize_kernels.h"
#include "esrgan_kernels.h"
#include "srgan_kernels.h"
#include "srgan_bwd_kernels.h"
#include "cgan_kernels.h"
#include "lpips_kernels.h"
#include "vgg_kernels.h"
#include "vgg_bwd_kernels.h"

#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <cmath>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <string>
#include <type_traits>
#include <vector>

#include "weight_store.h"

namespace {

using namespace cid;

struct ncclUniqueIdBytes { char internal[128]; };   // ncclUniqueId (rccl.h: NCCL_UNIQUE_ID_BYTES = 128), passed by value

enum Kind { HEAD, CONV, CONVT, TAIL };
struct LayerDef { const char* name; Kind kind; int cin, cout; bool pool = false; };   // pool: the 2x2 max-pool runs in this layer's epilogue
constexpr int NL = 12;
constexpr LayerDef kLayers[NL] = {
    {"down1.0", HEAD, 3, 64},          {"down1.2", CONV, 64, 64, true},  {"down2.0", CONV, 64, 128},
    {"down2.2", CONV, 128, 128, true}, {"bottleneck.0", CONV, 128, 256}, {"bottleneck.2", CONV, 256, 256},
    {"up2", CONVT, 256, 128},          {"upconv2.0", CONV, 256, 128},    {"upconv2.2", CONV, 128, 128},
    {"up1", CONVT, 128, 64},           {"upconv1.0", CONV, 128, 64},     {"upconv1.2", TAIL, 64, 3},
};
// MODE template argument of the GEMM-shaped kernels: 0 conv 3x3, 1 conv 3x3 + 2x2 pool, 2 transposed conv 2x2 stride 2
constexpr int mode_of(const LayerDef& L) { return L.kind == CONVT ? 2 : L.pool ? 1 : 0; }

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline unsigned long long cdiv_ull(unsigned long long a, unsigned long long b) { return (a + b - 1) / b; }

size_t ref_weight_count(const LayerDef& L) { return (size_t)L.cin * L.cout * (L.kind == CONVT ? 4 : 9); }
size_t packed_weight_count(const LayerDef& L) {
    switch (L.kind) {
        case HEAD: return 2 * 14 * 64;
        case TAIL: return 2 * 4 * 64 * 4;   // [chunk][group][lane][4], columns 27..31 stay zero
        default: return ref_weight_count(L);
    }
}

// float offsets of each layer's packed weights / bias inside the blob; segments 256-byte aligned
//   [direct-kernel segments][Winograd U of the eight 3x3 GEMM layers][reference-layout copy of all 24 tensors]
// The reference-layout copy makes the blob self-describing (state_dict() after a broadcast is exact: U is
// not invertible bit-for-bit).
struct BlobLayout {
    size_t w_off[NL], b_off[NL], u_off[NL], u42_off[NL], h_off[NL], raw_w_off[NL], raw_b_off[NL], tab_off[2], tab42_off[2], hz_off, s_off[NL], hzs_off, total;
    BlobLayout() {
        size_t o = 0;
        for (int l = 0; l < NL; ++l) {
            w_off[l] = o; o = align_up(o + packed_weight_count(kLayers[l]), 64);
            b_off[l] = o; o = align_up(o + kLayers[l].cout, 64);
        }
        for (int l = 0; l < NL; ++l) {
            u_off[l] = o;
            if (kLayers[l].kind == CONV) o = align_up(o + (size_t)kLayers[l].cin * kLayers[l].cout * 16, 64);
        }
        for (int l = 0; l < NL; ++l) {   // fp16-storage path: half weights (2 per float slot), in each kernel's fragment order
            h_off[l] = o;
            if (kLayers[l].kind == CONV || kLayers[l].kind == CONVT) o = align_up(o + (ref_weight_count(kLayers[l]) + 1) / 2, 64);
            if (kLayers[l].kind == TAIL) o = align_up(o + 4 * 64 * 8 / 2, 64);   // k_conv_tail_h: [4 k-steps][64 lanes][8] halfs
            if (kLayers[l].kind == HEAD) o = align_up(o + 4 * 64 * 8 / 2, 64);   // k_conv_head_h16: [4 channel groups][64 lanes][8] halfs
        }
        for (int l = 0; l < NL; ++l) {
            raw_w_off[l] = o; o = align_up(o + ref_weight_count(kLayers[l]), 64);
            raw_b_off[l] = o; o = align_up(o + kLayers[l].cout, 64);
        }
        tab_off[0] = o; o = align_up(o + wino_slot_table(32, 1, nullptr), 64);   // Winograd LDS slot tables, TC = 32 and 16
        tab_off[1] = o; o = align_up(o + wino_slot_table(16, 2, nullptr), 64);
        for (int l = 0; l < NL; ++l) {   // Winograd F(4x2,3x3): U at 24 positions
            u42_off[l] = o;
            if (kLayers[l].kind == CONV) o = align_up(o + (size_t)kLayers[l].cin * kLayers[l].cout * 24, 64);
        }
        tab42_off[0] = o; o = align_up(o + wino42_slot_table<8>(nullptr), 64);   // its LDS slot tables, TC = 8 and 4
        tab42_off[1] = o; o = align_up(o + wino42_slot_table<4>(nullptr), 64);
        hz_off = o; o = align_up(o + 3 * 2 * 64 * 8 / 2, 64);   // fp16 path, fused last layer: upconv1[2] as A fragments [2 row tiles][2 k-steps][64 lanes][8] halfs (room for three, as round 4's first form had)
        for (int l = 0; l < NL; ++l) {   // conv_algo = "split16": hi | lo | hi half pieces of the eight 3x3 layers' weights, in the order k_conv3x3_h16<F32IO> consumes them (27 halfs per weight)
            s_off[l] = o;
            if (kLayers[l].kind == CONV) o = align_up(o + ((size_t)kLayers[l].cin * kLayers[l].cout * 27 + 1) / 2, 64);
        }
        for (int l = 0; l < NL; ++l)   // split16: the two transposed convolutions' hi | lo | hi pieces, [block = (tap, 64 channels)][chunk][piece][cg][lane][8] halfs (12 halfs per weight)
            if (kLayers[l].kind == CONVT) { s_off[l] = o; o = align_up(o + ((size_t)kLayers[l].cin * kLayers[l].cout * 12 + 1) / 2, 64); }
        hzs_off = o; o = align_up(o + 2 * 2 * 2 * 64 * 8 / 2, 64);   // split16, fused last layer: upconv1[2] as A fragments [hi | lo][2 row tiles][2 k-steps][64 lanes][8] halfs
        total = o;
    }
};
const BlobLayout kBlob;

// The blob's segments in blob order, each with the alignment gap after it: what cid_packed_segment enumerates and what
// k_gen_pack (gen_pack_kernels.h) fills.  `count` = the elements (fp32 words, or halfs in the half families) that carry data;
// the rest of the segment is zero.
struct SegDef { size_t off; std::string name; GenPackFamily fam; int layer, src; size_t count; };
const std::vector<SegDef>& blob_segments() {
    static const std::vector<SegDef> segs = [] {
        std::vector<SegDef> v;
        for (int l = 0; l < NL; ++l) {
            const LayerDef& L = kLayers[l];
            const std::string n = L.name;
            const size_t nw = ref_weight_count(L);
            const GenPackFamily wf = L.kind == HEAD ? GP_W_HEAD : L.kind == TAIL ? GP_W_TAIL : L.kind == CONV ? GP_W_GEMM : L.cin == 128 ? GP_W_CONVT_S32 : GP_W_GEMM_T;
            v.push_back({kBlob.w_off[l], "w:" + n, wf, l, 2 * l, packed_weight_count(L)});
            v.push_back({kBlob.b_off[l], "b:" + n, GP_COPY, l, 2 * l + 1, (size_t)L.cout});
            v.push_back({kBlob.raw_w_off[l], "raw_w:" + n, GP_COPY, l, 2 * l, nw});
            v.push_back({kBlob.raw_b_off[l], "raw_b:" + n, GP_COPY, l, 2 * l + 1, (size_t)L.cout});
            if (L.kind == CONV) {
                v.push_back({kBlob.u_off[l], "u:" + n, GP_U, l, 2 * l, nw / 9 * 16});
                v.push_back({kBlob.u42_off[l], "u42:" + n, GP_U42, l, 2 * l, nw / 9 * 24});
                v.push_back({kBlob.h_off[l], "h:" + n, GP_H_CONV, l, 2 * l, nw});
                v.push_back({kBlob.s_off[l], "s16:" + n, GP_S_CONV, l, 2 * l, nw * 3});
            } else if (L.kind == CONVT) {
                v.push_back({kBlob.h_off[l], "h:" + n, GP_H_CONVT, l, 2 * l, nw});
                v.push_back({kBlob.s_off[l], "s16:" + n, GP_S_CONVT, l, 2 * l, nw * 3});
            } else {
                v.push_back({kBlob.h_off[l], "h:" + n, L.kind == HEAD ? GP_H_HEAD : GP_H_TAIL, l, 2 * l, (size_t)4 * 64 * 8});
            }
        }
        v.push_back({kBlob.tab_off[0], "tab:32", GP_TAB, 0, 0, (size_t)wino_slot_count(32, 1)});
        v.push_back({kBlob.tab_off[1], "tab:16", GP_TAB, 0, 1, (size_t)wino_slot_count(16, 2)});
        v.push_back({kBlob.tab42_off[0], "tab42:8", GP_TAB, 0, 2, (size_t)wino42_slot_table<8>(nullptr)});
        v.push_back({kBlob.tab42_off[1], "tab42:4", GP_TAB, 0, 3, (size_t)wino42_slot_table<4>(nullptr)});
        v.push_back({kBlob.hz_off, "hz", GP_HZ, NL - 1, 2 * (NL - 1), (size_t)2 * 2 * 64 * 8});
        v.push_back({kBlob.hzs_off, "hzs", GP_HZS, NL - 1, 2 * (NL - 1), (size_t)2 * 2 * 2 * 64 * 8});
        std::sort(v.begin(), v.end(), [](const SegDef& a, const SegDef& b) { return a.off < b.off; });
        if (v.size() > (size_t)GP_MAX_SEGS) std::abort();   // GenPackArgs::seg holds them all
        return v;
    }();
    return segs;
}

// The segment table in the form the pack code (gen_pack_kernels.h) reads, with the work items counted; no pointers yet.
const GenPackArgs& gen_pack_table() {
    static const GenPackArgs table = [] {
        const std::vector<SegDef>& segs = blob_segments();
        static_assert(sizeof(GenPackArgs) <= 4096, "kernel arguments");
        GenPackArgs a{};
        a.nseg = (int)segs.size();
        unsigned items = 0;
        for (int i = 0; i < a.nseg; ++i) {
            const LayerDef& L = kLayers[segs[i].layer];
            const size_t end = i + 1 < a.nseg ? segs[i + 1].off : kBlob.total;
            const unsigned nq = (unsigned)((end - segs[i].off) / 4);
            a.seg[i] = GenPackSeg{(unsigned)(segs[i].off / 4), nq, items, (unsigned)segs[i].count, (unsigned short)L.cin, (unsigned short)L.cout,
                                  (unsigned char)segs[i].fam, (unsigned char)segs[i].src};
            const unsigned tiles = (nq + 63) / 64, group = (unsigned)gp_group(segs[i].fam);
            if (group > 1 && (nq % 64 || tiles % group || segs[i].count != (size_t)nq * (segs[i].fam < GP_H_CONV ? 4 : 8))) std::abort();   // a grouped segment is whole groups, no padding
            items += tiles / group;
        }
        a.nitems = items;
        return a;
    }();
    return table;
}

// k_gen_pack's arguments: the parameter pointers and the segment table.
GenPackArgs gen_pack_args(const float* const* params, void* blob) {
    GenPackArgs a = gen_pack_table();
    for (int i = 0; i < CID_NUM_PARAMS; ++i) a.p[i] = params[i];
    a.blob = static_cast<uint4*>(blob);
    return a;
}

// The host pack: the segments that parameter tensor `src` feeds (kTables: the four LDS slot tables, which read no tensor), written
// into the host blob by the device pack's own code, every work item over its 64 lanes.  A segment's quads run up to the next
// segment's start, so the alignment gap after it is rewritten as zeros and nothing outside it is touched.
constexpr int kTables = -1;
void stage_segments(float* staging, int src, const float* data) {
    const GenPackArgs& a = gen_pack_table();
    for (int i = 0; i < a.nseg; ++i) {
        const GenPackSeg& s = a.seg[i];
        if (s.fam == GP_TAB ? src != kTables : s.src != src) continue;
        const unsigned items = (i + 1 < a.nseg ? a.seg[i + 1].t0 : a.nitems) - s.t0;
        for (unsigned t = 0; t < items; ++t)
            for (int lane = 0; lane < 64; ++lane)
                gen_pack_produce(s, data, t, lane, [staging](unsigned q, const unsigned (&v)[4]) { std::memcpy(staging + 4 * (size_t)q, v, 16); });
    }
}

struct Dims {
    int N, H, W, H1, W1, H2, W2, Hu2, Wu2, Hu1, Wu1;
};
bool make_dims(int N, int H, int W, Dims& d) {
    if (N < 1 || H < 4 || W < 4) return false;
    d.N = N; d.H = H; d.W = W;
    d.H1 = H / 2; d.W1 = W / 2; d.H2 = d.H1 / 2; d.W2 = d.W1 / 2;       // floor-mode pools, app.py:48,56
    d.Hu2 = 2 * d.H2; d.Wu2 = 2 * d.W2; d.Hu1 = 2 * d.Hu2; d.Wu1 = 2 * d.Wu2;  // x2 transposed convs, app.py:65,73
    return true;
}

// Why an [N,3,H,W] forward is not accepted, or nullptr.  Besides the reference's own limit (H, W >= 4: ATen raises "Output
// size is too small", app.py:80-103) there are two of this implementation's:
//   * the kernels address ONE image's activations through a raw buffer descriptor with 32-bit byte offsets, and a lane
//     that must deliver zeros (convolution padding, ragged tiles) carries the offset 0x7ffffff0, which has to lie beyond
//     the descriptor's range.  The widest per-image tensor is cat1 = [4*(H/4), 4*(W/4), 128] fp32 (512 bytes per pixel);
//   * tile decode divides by multiply-high with 32-bit reciprocals: exact while (tiles of the launch) x (tiles per image) < 2^32,
//     i.e. N x t^2 < 2^32 with t = the most tiles (or blocks) per image of any launch: every tiling in use is listed below.
// Larger inputs are an error (CID_ERR_SHAPE), never wrong results: split the batch, or the image into stripes
// (api.serve_u8 does).
constexpr unsigned long long kZeroSentinel = 0x7ffffff0ull;
const char* shape_error(int N, int H, int W, Dims& d) {
    if (!make_dims(N, H, W, d)) return "N >= 1 and H, W >= 4 required (output size is too small)";
    if ((unsigned long long)H * W * 512ull >= kZeroSentinel)
        return "image too large for one call: H*W must stay below 4,194,303 pixels (32-bit per-image addressing); split it into stripes";
    unsigned long long t0 = 0;
    const unsigned long long per_image[] = {
        cdiv_ull(W, 32) * cdiv_ull(H, 4), cdiv_ull(W, 16) * cdiv_ull(H, 8),          // k_wino42_conv: 8 x 2 / 4 x 4 tiles of 4x2 pixels
        cdiv_ull(W, 64) * cdiv_ull(H, 2), cdiv_ull(W, 32) * cdiv_ull(H, 4),          // k_wino64_conv: 32 x 1 / 16 x 2 tiles of 2x2 pixels
        cdiv_ull(W, TILE_W) * cdiv_ull(H, TILE_H),                                   // head, tail, k_gemm_conv, the fp16 kernels
        cdiv_ull((unsigned long long)H * W, THREADS),                                // k_conv_tail_z: one thread per pixel
    };
    for (unsigned long long t : per_image) t0 = t > t0 ? t : t0;
    if ((unsigned long long)N * t0 * t0 >= (1ull << 32)) return "batch x image too large for one call (split the batch)";
    return nullptr;
}

// activation arena (floats), NHWC
enum Buf { T0, CAT1, P1, T1, CAT2, P2, T2, BT, T3, D2, T4, NBUF };
struct Plan { size_t off[NBUF]; size_t total_bytes; };
Plan make_plan(const Dims& d) {
    const size_t s0 = (size_t)d.N * d.H * d.W, s1 = (size_t)d.N * d.H1 * d.W1, s2 = (size_t)d.N * d.H2 * d.W2;
    const size_t su2 = (size_t)d.N * d.Hu2 * d.Wu2, su1 = (size_t)d.N * d.Hu1 * d.Wu1;
    const size_t sz[NBUF] = {s0 * 64, su1 * 128, s1 * 64, s1 * 128, su2 * 256, s2 * 128, s2 * 256, s2 * 256, su2 * 128, su2 * 128, su1 * 64};
    Plan p; size_t o = 0;
    for (int b = 0; b < NBUF; ++b) { p.off[b] = o; o = align_up(o + sz[b], 64); }
    p.total_bytes = o * sizeof(float);
    return p;
}

}  // namespace

struct cid_handle_s : HandleBase {
    std::vector<float> staging;        // packed host blob
    bool have[NL][2];
    int dtype = CID_DTYPE_F32;         // storage type of activations/weights between the first and last kernel
    int tail_algo = CID_TAIL_FUSED;    // last layer: see cid_set_tail_algo
    int algo = CID_ALGO_WINOGRAD42;    // 3x3 GEMM layers: Winograd F(4x2,3x3) (default), Winograd F(2x2,3x3) or CID_ALGO_DIRECT (9-tap implicit GEMM)
    std::vector<hipEvent_t> tev;       // armed timing events, (NL+1) per forward
    int tev_forwards = 0, tev_used = 0;
    cid_handle_s() : staging(kBlob.total, 0.f) {
        std::memset(have, 0, sizeof(have));
        stage_segments(staging.data(), kTables, nullptr);
    }
};

namespace {

// A handle's three settings.  The null handle stands for the direct fp32 kernels with a separate last layer.
struct Config { int dtype, algo, tail; };
Config config_of(cid_handle_t h) {
    return h ? Config{h->dtype, h->algo, h->tail_algo} : Config{CID_DTYPE_F32, CID_ALGO_DIRECT, CID_TAIL_BANDS};
}

// The kernel family (and instantiation class) of one launch.  run_forward launches what select_kernel picks and
// cid_launch_kernel reports the name of the same pick.  Within a value, the shape still chooses the tile width (Winograd),
// walking or not (k_conv3x3_h16) and bands or tiles (TAIL_BANDS above T2_MAXW).
enum class Kern {
    HEAD, HEAD_H16,               // k_conv_head / k_conv_head_h16
    GEMM,                         // k_gemm_conv<CIN, COUT, MODE>: CID_ALGO_DIRECT, and up2 on the fp32 path
    CONVT_S32,                    // k_convt_s32: up1 on the fp32 path
    WINO64, WINO42,               // k_wino64_conv / k_wino42_conv
    SPLIT, SPLIT_PAIR,            // CID_ALGO_SPLIT16, k_conv3x3_h16<..., F32IO>: one / two column blocks per workgroup
    H16, CONVT_T16,               // fp16 storage: k_conv3x3_h16, k_convt_t16
    Z_WINO64, Z_WINO42, Z_SPLIT, Z_H16,   // upconv1[0] with upconv1[2]'s contraction in its epilogue: z planes out
    TAIL_BANDS, TAIL_TILES, TAIL_H,       // upconv1[2] as a launch of its own: k_conv_tail2, k_conv_tail, k_conv_tail_h
    TAIL_Z, TAIL_ZH,                      // the nine-tap sum over the z planes: k_conv_tail_z (fp32), k_conv_tail_zh (half)
};

Kern select_kernel(const Config& c, int i) {
    const LayerDef& L = kLayers[i];
    const bool f16 = c.dtype == CID_DTYPE_F16;
    // The fused form lives in the epilogue of upconv1[0]'s kernel: the Winograd and split-operand kernels on the fp32 path (not
    // the 9-tap direct one), k_conv3x3_h16 on the fp16-storage path (one 3x3 algorithm there, so always).
    const bool fused = c.tail == CID_TAIL_FUSED && (f16 || c.algo != CID_ALGO_DIRECT);
    switch (L.kind) {
        case HEAD: return f16 ? Kern::HEAD_H16 : Kern::HEAD;
        case TAIL:
            if (fused) return f16 ? Kern::TAIL_ZH : Kern::TAIL_Z;
            return f16 ? Kern::TAIL_H : c.tail == CID_TAIL_BANDS ? Kern::TAIL_BANDS : Kern::TAIL_TILES;
        case CONVT:
            if (f16) return Kern::CONVT_T16;
            if (c.algo == CID_ALGO_SPLIT16) return Kern::SPLIT_PAIR;
            return L.cin == 128 ? Kern::CONVT_S32 : Kern::GEMM;
        case CONV: break;
    }
    const bool z = fused && i == 10;
    if (f16) return z ? Kern::Z_H16 : Kern::H16;
    switch (c.algo) {
        case CID_ALGO_WINOGRAD64: return z ? Kern::Z_WINO64 : Kern::WINO64;
        case CID_ALGO_WINOGRAD42: return z ? Kern::Z_WINO42 : Kern::WINO42;
        case CID_ALGO_SPLIT16: return z ? Kern::Z_SPLIT : L.cout >= 128 ? Kern::SPLIT_PAIR : Kern::SPLIT;
        default: return Kern::GEMM;   // CID_ALGO_DIRECT
    }
}

// The symbol prefix cid_launch_kernel reports: enough of the template argument list to tell the launch's instantiation from
// the library's others (generator.launch_table and the tracked profiles match on it).
std::string kernel_name(const Config& c, int i) {
    const LayerDef& L = kLayers[i];
    const std::string dims = std::to_string(L.cin) + ", " + std::to_string(L.cout);
    const std::string mode = dims + ", " + std::to_string(mode_of(L)) + ",", pool = dims + (L.pool ? ", true," : ", false,");
    switch (select_kernel(c, i)) {
        case Kern::HEAD: return "k_conv_head";
        case Kern::HEAD_H16: return "k_conv_head_h16";
        case Kern::GEMM: return "k_gemm_conv<" + dims + ", " + std::to_string(mode_of(L));   // MODE is the last template argument: no comma
        case Kern::CONVT_S32: return "k_convt_s32<" + dims + ">";
        case Kern::WINO64: case Kern::Z_WINO64: return "k_wino64_conv<" + pool;
        case Kern::WINO42: case Kern::Z_WINO42: return "k_wino42_conv<" + pool;
        case Kern::SPLIT: case Kern::SPLIT_PAIR: return "k_conv3x3_h16<" + mode + " false, false, true,";
        case Kern::H16: return "k_conv3x3_h16<" + mode + (i == 10 ? " false," : "");   // upconv1[0] also has a ZOUT instance
        case Kern::CONVT_T16: return "k_convt_t16<" + dims + ">";
        case Kern::Z_SPLIT: return "k_conv3x3_h16<" + mode + " true, false, true,";
        case Kern::Z_H16: return "k_conv3x3_h16<" + mode + " true,";
        case Kern::TAIL_BANDS: case Kern::TAIL_TILES: return "k_conv_tail";
        case Kern::TAIL_H: return "k_conv_tail_h<";
        case Kern::TAIL_Z: return c.algo == CID_ALGO_SPLIT16 ? "k_conv_tail_z<" : "k_conv_tail";   // Winograd: the family prefix, as in the tracked profiles
        case Kern::TAIL_ZH: return "k_conv_tail_zh<";
    }
    return "";
}
// ... formatted once for every configuration, so that cid_launch_kernel can hand out pointers that stay valid
struct KernelNames {
    std::string s[2][CID_ALGO_SPLIT16 + 1][3][NL];
    KernelNames() {
        for (int dt = 0; dt < 2; ++dt)
            for (int algo = 0; algo <= CID_ALGO_SPLIT16; ++algo)
                for (int tail = 0; tail < 3; ++tail)
                    for (int i = 0; i < NL; ++i) s[dt][algo][tail][i] = kernel_name(Config{dt, algo, tail}, i);
    }
};
const KernelNames kKernelNames;

bool find_key(const char* key, int& layer, int& is_bias) {
    if (!key) return false;
    const std::string k(key);
    for (int l = 0; l < NL; ++l) {
        const std::string n(kLayers[l].name);
        if (k == n + ".weight") { layer = l; is_bias = 0; return true; }
        if (k == n + ".bias") { layer = l; is_bias = 1; return true; }
    }
    return false;
}

// The tile grid of a launch over N images of Hc x Wc computed pixels in tw x th tiles: the fields the kernels' tile decode
// reads.  The head and tail kernels then walk groups of tiles (tile_groups); the others deal tiles to the eight XCD groups.
template <typename A>
void set_tiles(A& a, int N, int Hc, int Wc, int tw, int th) {
    a.tiles_x = cdiv(Wc, tw); a.tiles_y = cdiv(Hc, th); a.tiles_total = N * a.tiles_x * a.tiles_y;
    a.rcp_x = tile_rcp(a.tiles_x); a.rcp_xy = tile_rcp(a.tiles_x * a.tiles_y);
    if constexpr (std::is_same_v<A, HeadArgs> || std::is_same_v<A, TailArgs>) tile_groups(a);
    else a.tiles_per_xcd = cdiv(a.tiles_total, 8);
}

// One GEMM-shaped layer's tensors, NHWC.  The arena regions are sized for fp32; the fp16-storage path keeps its half tensors
// in the front half of the same regions, and the split-operand kernels read fp32 through GemmConvArgsH's half pointers.
struct LayerIO {
    const float* in; int Hin, Win, in_ps;   // input image, pixel stride in_ps
    float* out; int out_ps, out_coff;       // output, pixel stride out_ps, from channel out_coff (a slice of a concat tensor)
    int Hc, Wc;                             // pixels computed (a transposed convolution: input pixels)
    int Hs, Ws;                             // pixels stored, the top-left crop of Hc x Wc (a skip tensor)
    float* pool;                            // the 2x2-pooled output of a pooling layer, else null
};
template <typename A>
void set_layer_io(A& a, int N, const LayerIO& io) {
    a.in = reinterpret_cast<decltype(a.in)>(io.in); a.out = reinterpret_cast<decltype(a.out)>(io.out);
    a.pool = reinterpret_cast<decltype(a.pool)>(io.pool);
    a.N = N; a.Hin = io.Hin; a.Win = io.Win; a.in_ps = io.in_ps;
    a.Hc = io.Hc; a.Wc = io.Wc; a.Hs = io.Hs; a.Ws = io.Ws; a.out_ps = io.out_ps; a.out_coff = io.out_coff;
}

// What every launch of one forward shares.
struct Ctx { hipStream_t s; const float* blob; int N; Config c; };

// Grid of a k_wino42_conv launch over `tiles_per_xcd` tiles per XCD group and NB column blocks.  Small launches: one workgroup
// per (tile, column block), a.walk = 0.  Once there are more items than the chip holds at a time — two workgroups per CU (LDS
// 75 KiB, <= 256 VGPRs) — the grid is what is resident and the workgroups WALK: a.walk = grid / 8 walkers per XCD group, each
// taking tiles local, local + walk, ... with all NB column blocks of a tile back to back.  CID_WINO42_WG_PER_CU (environment) and
// cid_debug_winograd_workgroups_per_cu (development / testing aids): 0 = never walk (the round-2 behaviour), k = k workgroups per CU.
// The environment values are clamped like the debug setters' (0 = never walk ... the occupancy the kernel's LDS use admits).
int env_wg_per_cu(const char* name, int dflt, int hi) {
    const char* e = std::getenv(name);
    if (!e) return dflt;
    const int v = std::atoi(e);
    return v < 0 ? 0 : v > hi ? hi : v;
}
int g_wino42_wg_per_cu = env_wg_per_cu("CID_WINO42_WG_PER_CU", 2, 2);
// k_conv3x3_h16, same meaning.  Default 0 since round 4: with the epilogue storing straight from the accumulators (no LDS staging, no barrier in front
// of it) one workgroup per item is FASTER than three walkers per CU on every layer that walked — same box, three boxes: forward +2.3...+2.8 %, down1.2 -7...-8 %,
// upconv1.0 -5.5...-6.7 %, upconv2.2 -2.6...-3.2 %, down2.2 -1.5...-2.6 % (profiles/r04_ab_f16_walk_vs_not.txt) — where round 3's kernels had gained 2.4 % from walking.
int g_half_wg_per_cu = env_wg_per_cu("CID_HALF_WG_PER_CU", 0, 3);
// CID_WINO42_XNB (environment, measurement aid): bit mask over the column-block counts NB (2, 4) whose walking launches give every XCD group ONE
// column block (a.walk < 0, wino42_kernels.h) instead of walking all NB blocks of a tile back to back.  Default 0: profiles/r04_xnb_experiment.txt.
int g_wino42_xnb = env_wg_per_cu("CID_WINO42_XNB", 0, 6);
// CU count of the CURRENT device (the one the launch goes to), cached per device id: a process may drive unlike devices.
int device_cus() {
    constexpr int MAXDEV = 64;
    static std::atomic<int> cache[MAXDEV];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= MAXDEV) return 256;
    int n = cache[dev].load(std::memory_order_relaxed);
    if (n > 0) return n;
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1) n = 256;
    cache[dev].store(n, std::memory_order_relaxed);
    return n;
}
int wino42_grid(WinoArgs& a, int nb) {
    const int per_cu = g_wino42_wg_per_cu;
    const int cus = device_cus();
    const int items = 8 * a.tiles_per_xcd * nb;
    const int walkers = per_cu * cus / 8;                    // per XCD group
    a.walk = 0;
    // Walkers are indexed by TILE (a walker runs all nb column blocks of its tiles back to back), so walking needs at least one
    // tile per walker: with fewer, only tiles_per_xcd of the slots would work, each nb items deep, where one item per workgroup
    // spreads the same items over every CU (mid-size batches, N = 17..48 on the bottleneck layers).
    if (per_cu <= 0 || walkers < 1 || items <= 8 * walkers || a.tiles_per_xcd < walkers) return items;   // same-box against round 3's rule: profiles/r04_ab_midbatch_walk_rule.txt
    a.walk = walkers;
    if ((nb == 2 || nb == 4) && (g_wino42_xnb & nb)) {        // one column block per XCD group: 8 / nb tile ranges
        a.tiles_per_xcd = cdiv(a.tiles_total, 8 / nb);
        a.walk = -walkers;
    }
    return 8 * walkers;
}

template <int CIN, int COUT, int MODE>
hipError_t launch_gemm(const Ctx& x, int layer, const LayerIO& io) {
    GemmConvArgs a;
    set_layer_io(a, x.N, io);
    a.w = x.blob + kBlob.w_off[layer]; a.bias = x.blob + kBlob.b_off[layer];
    set_tiles(a, x.N, io.Hc, io.Wc, TILE_W, TILE_H);
    constexpr int NB = (MODE == 2 ? 4 * COUT : COUT) / NTILE;
    hipLaunchKernelGGL((k_gemm_conv<CIN, COUT, MODE>), dim3(8 * a.tiles_per_xcd * NB), dim3(THREADS), 0, x.s, a);
    return hipGetLastError();
}

// up1 on the fp32 path: streaming form, persistent workgroups (two per CU) over runs of TP input pixels
template <int CIN, int COUT>
hipError_t launch_convt_s32(const Ctx& x, int layer, const LayerIO& io) {
    using CG = ConvTGeom32<CIN, COUT>;
    GemmConvArgs a;
    set_layer_io(a, x.N, io);
    a.w = x.blob + kBlob.w_off[layer]; a.bias = x.blob + kBlob.b_off[layer];
    a.tiles_x = (io.Hin * io.Win + CG::TP - 1) / CG::TP; a.tiles_y = 1; a.tiles_total = x.N * a.tiles_x; a.tiles_per_xcd = 0;
    a.rcp_x = tile_rcp(a.tiles_x); a.rcp_xy = tile_rcp(io.Win);
    const int wgs = device_cus() * 2;
    hipLaunchKernelGGL((k_convt_s32<CIN, COUT>), dim3(a.tiles_total < wgs ? a.tiles_total : wgs), dim3(THREADS), 0, x.s, a);
    return hipGetLastError();
}

// The Winograd kernels' arguments.  ZOUT (upconv1[0] only): the channel contraction of upconv1[2] folded into the epilogue,
// z planes into io.out instead of the 64-channel tensor.
template <bool ZOUT>
WinoArgs wino_args(const Ctx& x, int layer, const LayerIO& io, size_t u_off) {
    WinoArgs a;
    set_layer_io(a, x.N, io);
    a.u = x.blob + u_off; a.bias = x.blob + kBlob.b_off[layer];
    a.zw = ZOUT ? x.blob + kBlob.w_off[11] : nullptr; a.zout = ZOUT ? io.out : nullptr;
    if (ZOUT) a.out = nullptr;
    a.walk = 0;
    return a;
}

// 32 tile-columns (64 pixels) per workgroup when the rows are wide enough, else 16 x 2 tile-rows
template <int CIN, int COUT, bool POOL, bool ZOUT>
hipError_t launch_wino64(const Ctx& x, int layer, const LayerIO& io) {
    WinoArgs a = wino_args<ZOUT>(x, layer, io, kBlob.u_off[layer]);
    const bool wide = io.Wc > 32;
    a.slot_tab = reinterpret_cast<const unsigned*>(x.blob + kBlob.tab_off[wide ? 0 : 1]);
    set_tiles(a, x.N, io.Hc, io.Wc, wide ? 64 : 32, wide ? 2 : 4);   // TC tile-columns of 2x2 pixels, 32 / TC tile-rows
    const dim3 grid(8 * a.tiles_per_xcd * (COUT / WN2));
    if (wide) hipLaunchKernelGGL((k_wino64_conv<CIN, COUT, POOL, 32, ZOUT>), grid, dim3(THREADS), 0, x.s, a);
    else hipLaunchKernelGGL((k_wino64_conv<CIN, COUT, POOL, 16, ZOUT>), grid, dim3(THREADS), 0, x.s, a);
    return hipGetLastError();
}

// 16 tiles of 4x2 pixels per workgroup: 8 x 2 (32x4 pixels), or 4 x 4 (16x8) for rows of 16 pixels or fewer.
// 16 x 1 (64x2 pixels) fetches 4 input rows for 2 of output: same-box 24.4k images/s against 24.8k (8 x 2) and 24.7k (4 x 4 everywhere)
template <int CIN, int COUT, bool POOL, bool ZOUT>
hipError_t launch_wino42(const Ctx& x, int layer, const LayerIO& io) {
    WinoArgs a = wino_args<ZOUT>(x, layer, io, kBlob.u42_off[layer]);
    const bool wide = io.Wc > 16;
    a.slot_tab = reinterpret_cast<const unsigned*>(x.blob + kBlob.tab42_off[wide ? 0 : 1]);
    set_tiles(a, x.N, io.Hc, io.Wc, wide ? 32 : 16, wide ? 4 : 8);   // TC tile-columns of 4x2 pixels, 16 / TC tile-rows
    const dim3 grid(wino42_grid(a, COUT / WN2));
    if (wide) hipLaunchKernelGGL((k_wino42_conv<CIN, COUT, POOL, 8, ZOUT>), grid, dim3(THREADS), 0, x.s, a);
    else hipLaunchKernelGGL((k_wino42_conv<CIN, COUT, POOL, 4, ZOUT>), grid, dim3(THREADS), 0, x.s, a);
    return hipGetLastError();
}

// conv_algo "split16": split-operand convolution on the fp16 MFMA, fp32 tensors in and out (conv_kernels_f16.h, F32IO): one
// (8x32-pixel tile, 64-channel column block) per workgroup, or two column blocks from one staging of the input tile (PAIR).
// A transposed convolution's column blocks are (tap, 64 channels) over tiles of its INPUT.  ZOUT: `out` = the 27 fp32 z
// planes, `pool` = upconv1[2]'s hi | lo fragments.
template <int CIN, int COUT, int MODE, bool ZOUT, bool PAIR>
hipError_t launch_split16(const Ctx& x, int layer, const LayerIO& io) {
    if (io.in_ps != CIN) return hipErrorInvalidValue;   // the kernel takes the pixel stride of its input as CIN (true of every layer of this network)
    GemmConvArgsH a;
    set_layer_io(a, x.N, io);
    a.w = reinterpret_cast<const _Float16*>(x.blob + kBlob.s_off[layer]); a.bias = x.blob + kBlob.b_off[layer];
    if (ZOUT) a.pool = const_cast<_Float16*>(reinterpret_cast<const _Float16*>(x.blob + kBlob.hzs_off));
    set_tiles(a, x.N, io.Hc, io.Wc, TILE_W, TILE_H);
    a.walk = 0;
    constexpr int NB = (MODE == 2 ? 4 * COUT : COUT) / NTILE / (PAIR ? 2 : 1);
    hipLaunchKernelGGL((k_conv3x3_h16<CIN, COUT, MODE, ZOUT, false, true, PAIR>), dim3(8 * a.tiles_per_xcd * NB), dim3(THREADS), 0, x.s, a);
    return hipGetLastError();
}

// The fp16-storage path: k_conv3x3_h16 (MODE 0/1; ZOUT: `out` = the z planes, `pool` = the last layer's weights, read only)
// or k_convt_t16 (MODE 2).
template <int CIN, int COUT, int MODE, bool ZOUT>
hipError_t launch_gemm_h(const Ctx& x, int layer, const LayerIO& io) {
    GemmConvArgsH a;
    set_layer_io(a, x.N, io);
    a.w = reinterpret_cast<const _Float16*>(x.blob + kBlob.h_off[layer]); a.bias = x.blob + kBlob.b_off[layer];
    if (ZOUT) a.pool = const_cast<_Float16*>(reinterpret_cast<const _Float16*>(x.blob + kBlob.hz_off));
    set_tiles(a, x.N, io.Hc, io.Wc, TILE_W, TILE_H);
    constexpr int NB = (MODE == 2 ? 4 * COUT : COUT) / NTILE;
    a.walk = 0;
    if constexpr (MODE == 2 && !ZOUT) {
        // streaming form: persistent workgroups (two waves per SIMD: 2 per CU of four waves, 1 of eight) over runs of TP input pixels
        using CG = ConvTGeom<CIN, COUT>;
        a.tiles_x = (io.Hin * io.Win + CG::TP - 1) / CG::TP; a.tiles_total = x.N * a.tiles_x;
        a.rcp_x = tile_rcp(a.tiles_x); a.rcp_xy = tile_rcp(io.Win);
        const int wgs = device_cus() * 2 / CG::CB;
        hipLaunchKernelGGL((k_convt_t16<CIN, COUT>), dim3(a.tiles_total < wgs ? a.tiles_total : wgs), dim3(64 * CG::NW), 0, x.s, a);
    } else if constexpr (MODE != 2) {
        if (io.in_ps != CIN) return hipErrorInvalidValue;   // k_conv3x3_h16 takes the pixel stride of its input as CIN (true of every layer of this network)
        // walking workgroups (conv_kernels_f16.h): three per CU (47 KiB of LDS, <= 168 VGPRs) once there are more items than that —
        // on the layers with CIN <= 128, where an item is short beside its prologue (same-box: down1.2 -15 %, down2.0 -11 %, the
        // CIN = 128 layers -0.3...-1.5 %).  With CIN = 256 walking LOSES 3-5 %: a tile's NB column blocks then run one after the
        // other in one workgroup and the 174 KB halo tile of the second pass has left the XCD's L2 (96 walkers x 174 KB), while
        // sibling workgroups dispatched back to back share one fetch (profiles/r03_ab_f16_walk.txt).
        int grid = 8 * a.tiles_per_xcd * NB;
        const int walkers = g_half_wg_per_cu * device_cus() / 8;
        if (CIN <= 128 && g_half_wg_per_cu > 0 && walkers >= 1 && grid > 8 * walkers && a.tiles_per_xcd >= walkers) { a.walk = walkers; grid = 8 * walkers; }   // >= one tile per walker, as in wino42_grid
        // the pooling launches (MODE 1) never walk: their walking variants were the last kernels of the library with spilled registers (4 VGPRs, 20 B of
        // scratch per lane) and walking is slower than one item per workgroup on them by the widest margin (-7...-10 % on down1.2)
        if constexpr (MODE == 0) {
            if (a.walk) { hipLaunchKernelGGL((k_conv3x3_h16<CIN, COUT, MODE, ZOUT, true>), dim3(grid), dim3(THREADS), 0, x.s, a); return hipGetLastError(); }
        }
        a.walk = 0; grid = 8 * a.tiles_per_xcd * NB;
        hipLaunchKernelGGL((k_conv3x3_h16<CIN, COUT, MODE, ZOUT, false>), dim3(grid), dim3(THREADS), 0, x.s, a);
    }
    return hipGetLastError();
}

// One GEMM-shaped layer (launches 1..10) with the kernel select_kernel picks for it.  Only the instantiations a layer can
// reach are compiled: upconv1[0] is the one layer with a fused (ZOUT) form, up1 the one on k_convt_s32.
template <int LAYER>
hipError_t launch_layer(const Ctx& x, const LayerIO& io) {
    constexpr int CIN = kLayers[LAYER].cin, COUT = kLayers[LAYER].cout, MODE = mode_of(kLayers[LAYER]);
    constexpr bool CONV = MODE != 2, Z = LAYER == 10, S32 = MODE == 2 && CIN == 128;
    switch (select_kernel(x.c, LAYER)) {
        case Kern::GEMM: if constexpr (!S32) return launch_gemm<CIN, COUT, MODE>(x, LAYER, io); break;
        case Kern::CONVT_S32: if constexpr (S32) return launch_convt_s32<CIN, COUT>(x, LAYER, io); break;
        case Kern::WINO64: if constexpr (CONV) return launch_wino64<CIN, COUT, MODE == 1, false>(x, LAYER, io); break;
        case Kern::WINO42: if constexpr (CONV) return launch_wino42<CIN, COUT, MODE == 1, false>(x, LAYER, io); break;
        case Kern::SPLIT: if constexpr (CONV && COUT < 128) return launch_split16<CIN, COUT, MODE, false, false>(x, LAYER, io); break;
        case Kern::SPLIT_PAIR: if constexpr (!CONV || COUT >= 128) return launch_split16<CIN, COUT, MODE, false, true>(x, LAYER, io); break;
        case Kern::H16: if constexpr (CONV) return launch_gemm_h<CIN, COUT, MODE, false>(x, LAYER, io); break;
        case Kern::CONVT_T16: if constexpr (!CONV) return launch_gemm_h<CIN, COUT, MODE, false>(x, LAYER, io); break;
        case Kern::Z_WINO64: if constexpr (Z) return launch_wino64<CIN, COUT, false, true>(x, LAYER, io); break;
        case Kern::Z_WINO42: if constexpr (Z) return launch_wino42<CIN, COUT, false, true>(x, LAYER, io); break;
        case Kern::Z_SPLIT: if constexpr (Z) return launch_split16<CIN, COUT, MODE, true, false>(x, LAYER, io); break;
        case Kern::Z_H16: if constexpr (Z) return launch_gemm_h<CIN, COUT, MODE, true>(x, LAYER, io); break;
        default: break;
    }
    return hipErrorInvalidValue;   // not a kernel of this layer
}

// down1[0]: Conv 3->64 + ReLU, the caller's image placed at `src` inside the H x W network input -> NHWC t0
hipError_t launch_head(const Ctx& x, const void* in, bool u8, const Window& src, float* out, int H, int W) {
    const bool f16 = select_kernel(x.c, 0) == Kern::HEAD_H16;
    HeadArgs a;
    a.in = in; a.w = x.blob + (f16 ? kBlob.h_off[0] : kBlob.w_off[0]); a.bias = x.blob + kBlob.b_off[0]; a.out = out;
    a.N = x.N; a.H = H; a.W = W; a.src = src;
    set_tiles(a, x.N, H, W, TILE_W, TILE_H);
    const dim3 grid(8 * a.groups_per_xcd);
    if (u8 && f16) hipLaunchKernelGGL((k_conv_head_h16<true>), grid, dim3(THREADS), 0, x.s, a);
    else if (u8) hipLaunchKernelGGL((k_conv_head<true>), grid, dim3(THREADS), 0, x.s, a);
    else if (f16) hipLaunchKernelGGL((k_conv_head_h16<false>), grid, dim3(THREADS), 0, x.s, a);
    else hipLaunchKernelGGL((k_conv_head<false>), grid, dim3(THREADS), 0, x.s, a);
    return hipGetLastError();
}

// upconv1[2] + tanh from the t4 region (H x W) -> the `crop` window of the caller's tensor: the last layer itself on upconv1[0]'s
// 64 channels, or the nine-tap shifted sum + bias + tanh over the z planes a fused upconv1[0] left there.
hipError_t launch_tail(const Ctx& x, const float* t4, void* out, bool u8, const Window& crop, int H, int W) {
    const Kern k = select_kernel(x.c, 11);
    const float* bias = x.blob + kBlob.b_off[11];
    if (k == Kern::TAIL_Z || k == Kern::TAIL_ZH) {   // one thread per pixel
        TailZArgs a;
        a.z = t4; a.bias = bias; a.out = out; a.crop = crop; a.N = x.N; a.H = H; a.W = W;
        a.blocks_per_image = cdiv(H * W, THREADS);
        a.rcp_w = tile_rcp((unsigned)W); a.rcp_blocks = tile_rcp((unsigned)a.blocks_per_image);
        const dim3 grid(x.N * a.blocks_per_image);
        if (k == Kern::TAIL_ZH && u8) hipLaunchKernelGGL((k_conv_tail_zh<true>), grid, dim3(THREADS), 0, x.s, a);
        else if (k == Kern::TAIL_ZH) hipLaunchKernelGGL((k_conv_tail_zh<false>), grid, dim3(THREADS), 0, x.s, a);
        else if (u8) hipLaunchKernelGGL((k_conv_tail_z<true>), grid, dim3(THREADS), 0, x.s, a);
        else hipLaunchKernelGGL((k_conv_tail_z<false>), grid, dim3(THREADS), 0, x.s, a);
        return hipGetLastError();
    }
    if (k == Kern::TAIL_BANDS && W <= T2_MAXW) {   // row-band kernel: z once per pixel
        Tail2Args a;
        a.in = t4; a.w = x.blob + kBlob.w_off[11]; a.bias = bias; a.out = out; a.crop = crop;
        a.N = x.N; a.H = H; a.W = W;
        tail2_plan(a);
        if (u8) hipLaunchKernelGGL((k_conv_tail2<true>), dim3(a.groups_total), dim3(THREADS), 0, x.s, a);
        else hipLaunchKernelGGL((k_conv_tail2<false>), dim3(a.groups_total), dim3(THREADS), 0, x.s, a);
        return hipGetLastError();
    }
    // 8x32 tiles with halo: TAIL_TILES, TAIL_BANDS on images wider than T2_MAXW, and the fp16-storage path (TAIL_H)
    const bool f16 = k == Kern::TAIL_H;
    TailArgs a;
    a.in = t4; a.w = x.blob + (f16 ? kBlob.h_off[11] : kBlob.w_off[11]); a.bias = bias; a.out = out; a.crop = crop;
    a.N = x.N; a.H = H; a.W = W;
    set_tiles(a, x.N, H, W, TILE_W, TILE_H);
    const dim3 grid(8 * a.groups_per_xcd);
    if (u8 && f16) hipLaunchKernelGGL((k_conv_tail_h<true>), grid, dim3(THREADS), 0, x.s, a);
    else if (u8) hipLaunchKernelGGL((k_conv_tail<true, false>), grid, dim3(THREADS), 0, x.s, a);
    else if (f16) hipLaunchKernelGGL((k_conv_tail_h<false>), grid, dim3(THREADS), 0, x.s, a);
    else hipLaunchKernelGGL((k_conv_tail<false, false>), grid, dim3(THREADS), 0, x.s, a);
    return hipGetLastError();
}

// (H, W) = the network input.  `src` places the caller's image inside it (the band around it is uint8 0 = -1.0 normalised), `crop`
// is the window of the network output the caller's tensor receives; null = identity (no padding, whole output).
// `ev`: NL + 1 events to record around the launches; null = the next armed set of cid_timing_begin, if there is one.
int run_forward(cid_handle_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, void* ws, size_t ws_bytes,
                hipStream_t s, hipEvent_t* ev = nullptr, const Window* src_win = nullptr, const Window* crop_win = nullptr,
                const Config* cfg = nullptr) {
    if (!h) return CID_ERR_INVALID;
    if (!in || !out || !ws) return h->fail(CID_ERR_INVALID, "cid_forward: null pointer");
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, "cid_forward: no device weights attached (call cid_upload_weights or cid_attach_weights)");
    Dims d;
    if (const char* why = shape_error(N, H, W, d)) {
        char m[256];
        std::snprintf(m, sizeof m, "cid_forward: input [%d,3,%d,%d] not accepted: %s", N, H, W, why);
        return h->fail(CID_ERR_SHAPE, m);
    }
    const Plan p = make_plan(d);
    if (ws_bytes < p.total_bytes) return h->fail(CID_ERR_WORKSPACE, "cid_forward: workspace smaller than cid_workspace_bytes()");
    if ((in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) || (out_fmt != CID_FMT_F32_NCHW && out_fmt != CID_FMT_U8_NHWC))
        return h->fail(CID_ERR_INVALID, "cid_forward: unknown tensor format");
    if (((uintptr_t)ws & 255) || ((uintptr_t)h->dev_blob & 255) || (in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)))
        return h->fail(CID_ERR_WORKSPACE, "cid_forward: workspace/weights must be 256-byte aligned, fp32 input 4-byte aligned");
    const bool armed = !ev && !cfg && h->tev_used < h->tev_forwards;
    if (armed) ev = h->tev.data() + (size_t)h->tev_used * (NL + 1);
    float* base = static_cast<float*>(ws);
    float* B[NBUF];
    for (int b = 0; b < NBUF; ++b) B[b] = base + p.off[b];
    const Ctx x{s, h->dev_blob, N, cfg ? *cfg : config_of(h)};   // cfg: this call's configuration in place of the handle's (cid_forward_saved)
    hipError_t e = hipSuccess;
    int li = 0;
#define STEP(call)                                                                         \
    do {                                                                                   \
        if (ev && hipEventRecord(ev[li], s) != hipSuccess) e = hipErrorUnknown;            \
        if (e == hipSuccess) e = (call);                                                   \
        if (e != hipSuccess) {                                                             \
            return h->fail(CID_ERR_HIP, std::string("launch '") + kLayers[li].name + "' failed: " + hipGetErrorString(e)); \
        }                                                                                  \
        ++li;                                                                              \
    } while (0)

    // down1[0]: Conv 3->64 + ReLU, NCHW in -> NHWC t0                                    app.py:43-44
    STEP(launch_head(x, in, in_fmt == CID_FMT_U8_NHWC, src_win ? *src_win : Window{0, 0, H, W}, B[T0], H, W));
    // down1[2] + ReLU -> e1 into cat1[:, 64:128] (cropped to Hu1 x Wu1), pool1 -> p1     app.py:45-48,97-100
    STEP(launch_layer<1>(x, {.in = B[T0], .Hin = H, .Win = W, .in_ps = 64, .out = B[CAT1], .out_ps = 128, .out_coff = 64,
                             .Hc = 2 * d.H1, .Wc = 2 * d.W1, .Hs = d.Hu1, .Ws = d.Wu1, .pool = B[P1]}));
    // down2[0] + ReLU                                                                    app.py:51-52
    STEP(launch_layer<2>(x, {.in = B[P1], .Hin = d.H1, .Win = d.W1, .in_ps = 64, .out = B[T1], .out_ps = 128, .out_coff = 0,
                             .Hc = d.H1, .Wc = d.W1, .Hs = d.H1, .Ws = d.W1, .pool = nullptr}));
    // down2[2] + ReLU -> e2 into cat2[:, 128:256] (cropped), pool2 -> p2                 app.py:53-56,90-93
    STEP(launch_layer<3>(x, {.in = B[T1], .Hin = d.H1, .Win = d.W1, .in_ps = 128, .out = B[CAT2], .out_ps = 256, .out_coff = 128,
                             .Hc = d.Hu2, .Wc = d.Wu2, .Hs = d.Hu2, .Ws = d.Wu2, .pool = B[P2]}));
    // bottleneck                                                                         app.py:59-62
    STEP(launch_layer<4>(x, {.in = B[P2], .Hin = d.H2, .Win = d.W2, .in_ps = 128, .out = B[T2], .out_ps = 256, .out_coff = 0,
                             .Hc = d.H2, .Wc = d.W2, .Hs = d.H2, .Ws = d.W2, .pool = nullptr}));
    STEP(launch_layer<5>(x, {.in = B[T2], .Hin = d.H2, .Win = d.W2, .in_ps = 256, .out = B[BT], .out_ps = 256, .out_coff = 0,
                             .Hc = d.H2, .Wc = d.W2, .Hs = d.H2, .Ws = d.W2, .pool = nullptr}));
    // up2: ConvT 256->128 -> cat2[:, 0:128]                                              app.py:65,89
    STEP(launch_layer<6>(x, {.in = B[BT], .Hin = d.H2, .Win = d.W2, .in_ps = 256, .out = B[CAT2], .out_ps = 256, .out_coff = 0,
                             .Hc = d.H2, .Wc = d.W2, .Hs = d.H2, .Ws = d.W2, .pool = nullptr}));
    // upconv2                                                                            app.py:67-70
    STEP(launch_layer<7>(x, {.in = B[CAT2], .Hin = d.Hu2, .Win = d.Wu2, .in_ps = 256, .out = B[T3], .out_ps = 128, .out_coff = 0,
                             .Hc = d.Hu2, .Wc = d.Wu2, .Hs = d.Hu2, .Ws = d.Wu2, .pool = nullptr}));
    STEP(launch_layer<8>(x, {.in = B[T3], .Hin = d.Hu2, .Win = d.Wu2, .in_ps = 128, .out = B[D2], .out_ps = 128, .out_coff = 0,
                             .Hc = d.Hu2, .Wc = d.Wu2, .Hs = d.Hu2, .Ws = d.Wu2, .pool = nullptr}));
    // up1: ConvT 128->64 -> cat1[:, 0:64]                                                app.py:73,96
    STEP(launch_layer<9>(x, {.in = B[D2], .Hin = d.Hu2, .Win = d.Wu2, .in_ps = 128, .out = B[CAT1], .out_ps = 128, .out_coff = 0,
                             .Hc = d.Hu2, .Wc = d.Wu2, .Hs = d.Hu2, .Ws = d.Wu2, .pool = nullptr}));
    // upconv1[0] + ReLU -> t4; fused tail: upconv1[2]'s channel contraction in its epilogue, z planes into t4    app.py:75-77
    STEP(launch_layer<10>(x, {.in = B[CAT1], .Hin = d.Hu1, .Win = d.Wu1, .in_ps = 128, .out = B[T4], .out_ps = 64, .out_coff = 0,
                              .Hc = d.Hu1, .Wc = d.Wu1, .Hs = d.Hu1, .Ws = d.Wu1, .pool = nullptr}));
    // upconv1[2] + tanh, NHWC t4 -> NCHW out                                             app.py:77,103
    STEP(launch_tail(x, B[T4], out, out_fmt == CID_FMT_U8_NHWC, crop_win ? *crop_win : Window{0, 0, d.Hu1, d.Wu1}, d.Hu1, d.Wu1));
#undef STEP
    if (ev && hipEventRecord(ev[NL], s) != hipSuccess) return h->fail(CID_ERR_HIP, "hipEventRecord failed");
    if (armed) ++h->tev_used;
    return CID_OK;
}

}  // namespace

extern "C" {

const char* cid_version(void) { return "cid 0.4.0 (gfx950, fp32 MFMA: Winograd F(4x2,3x3) / F(2x2,3x3) + implicit GEMM; fp16-storage path: 16x16x32 MFMA)"; }

int cid_create(cid_handle_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = new (std::nothrow) cid_handle_s();
    return *out ? CID_OK : CID_ERR_INVALID;
}

void cid_destroy(cid_handle_t h) {
    if (h) for (hipEvent_t e : h->tev) (void)hipEventDestroy(e);
    delete h;
}

const char* cid_last_error(cid_handle_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_param_key(int i) {
    static std::string keys[CID_NUM_PARAMS];
    if (i < 0 || i >= CID_NUM_PARAMS) return nullptr;
    if (keys[i].empty()) keys[i] = std::string(kLayers[i / 2].name) + ((i & 1) ? ".bias" : ".weight");
    return keys[i].c_str();
}

int cid_set_weight(cid_handle_t h, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!h) return CID_ERR_INVALID;
    if (!key || !data || !shape) return h->fail(CID_ERR_INVALID, "cid_set_weight: null argument");
    int l, is_bias;
    if (!find_key(key, l, is_bias)) return h->fail(CID_ERR_KEY, std::string("unexpected key '") + key + "' in state_dict");
    const LayerDef& L = kLayers[l];
    int64_t want[4]; int wn;
    if (is_bias) { want[0] = L.cout; wn = 1; }
    else if (L.kind == CONVT) { want[0] = L.cin; want[1] = L.cout; want[2] = 2; want[3] = 2; wn = 4; }
    else { want[0] = L.cout; want[1] = L.cin; want[2] = 3; want[3] = 3; wn = 4; }
    bool ok = ndim == wn;
    for (int i = 0; ok && i < wn; ++i) ok = shape[i] == want[i];
    if (!ok) {
        std::string m = std::string("size mismatch for ") + key + ": expected [";
        for (int i = 0; i < wn; ++i) m += (i ? "," : "") + std::to_string(want[i]);
        m += "], got [";
        for (int i = 0; i < ndim; ++i) m += (i ? "," : "") + std::to_string(shape[i]);
        return h->fail(CID_ERR_SHAPE, m + "]");
    }
    stage_segments(h->staging.data(), 2 * l + is_bias, data);   // every layout of this tensor, the reference-layout copy included
    h->have[l][is_bias] = true;
    return CID_OK;
}

int cid_get_weight(cid_handle_t h, const char* key, float* out, size_t count) {
    if (!h) return CID_ERR_INVALID;
    if (!key || !out) return h->fail(CID_ERR_INVALID, "cid_get_weight: null argument");
    int l, is_bias;
    if (!find_key(key, l, is_bias)) return h->fail(CID_ERR_KEY, std::string("unknown key '") + key + "'");
    const LayerDef& L = kLayers[l];
    const size_t need = is_bias ? (size_t)L.cout : ref_weight_count(L);
    if (count != need) return h->fail(CID_ERR_SHAPE, std::string("cid_get_weight: wrong element count for ") + key);
    // the blob carries a reference-layout copy of every tensor (the Winograd U is not invertible bit-for-bit)
    std::memcpy(out, h->staging.data() + (is_bias ? kBlob.raw_b_off[l] : kBlob.raw_w_off[l]), sizeof(float) * need);
    return CID_OK;
}

int cid_missing_weights(cid_handle_t h, int* missing) {
    if (!h || !missing) return CID_ERR_INVALID;
    int m = 0;
    for (int l = 0; l < NL; ++l) m += !h->have[l][0] + !h->have[l][1];
    *missing = m;
    return CID_OK;
}

size_t cid_packed_weights_bytes(void) { return kBlob.total * sizeof(float); }

int cid_upload_weights(cid_handle_t h, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!device_blob) return h->fail(CID_ERR_INVALID, "cid_upload_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return h->fail(CID_ERR_WORKSPACE, "cid_upload_weights: blob must be 256-byte aligned");
    return h->upload_blob("cid_upload_weights: ", device_blob, h->staging.data(), kBlob.total, stream);
}

int cid_pack_weights_device(cid_handle_t h, const float* const* dev_params, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!dev_params || !device_blob) return h->fail(CID_ERR_INVALID, "cid_pack_weights_device: null pointer");
    for (int i = 0; i < CID_NUM_PARAMS; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3))
            return h->fail(CID_ERR_INVALID, "cid_pack_weights_device: null or misaligned parameter pointer");
    if ((uintptr_t)device_blob & 255) return h->fail(CID_ERR_WORKSPACE, "cid_pack_weights_device: blob must be 256-byte aligned");
    const GenPackArgs a = gen_pack_args(dev_params, device_blob);
    hipLaunchKernelGGL(k_gen_pack, dim3((a.nitems + GP_THREADS / 64 - 1) / (GP_THREADS / 64)), dim3(GP_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return h->fail(CID_ERR_HIP, "cid_pack_weights_device: launch failed");
    h->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_packed_segment(int index, const char** name, size_t* offset_bytes, size_t* bytes) {
    const std::vector<SegDef>& segs = blob_segments();
    if (index < 0 || (size_t)index >= segs.size()) return CID_ERR_INVALID;
    const size_t end = (size_t)index + 1 < segs.size() ? segs[index + 1].off : kBlob.total;
    if (name) *name = segs[index].name.c_str();
    if (offset_bytes) *offset_bytes = segs[index].off * sizeof(float);
    if (bytes) *bytes = (end - segs[index].off) * sizeof(float);
    return CID_OK;
}

int cid_export_packed(cid_handle_t h, void* host_out, size_t bytes) {
    if (!h) return CID_ERR_INVALID;
    if (!host_out) return h->fail(CID_ERR_INVALID, "cid_export_packed: null pointer");
    if (bytes != kBlob.total * sizeof(float)) return h->fail(CID_ERR_SHAPE, "cid_export_packed: size != cid_packed_weights_bytes()");
    std::memcpy(host_out, h->staging.data(), bytes);
    return CID_OK;
}

int cid_import_packed(cid_handle_t h, const void* host_in, size_t bytes) {
    if (!h) return CID_ERR_INVALID;
    if (!host_in) return h->fail(CID_ERR_INVALID, "cid_import_packed: null pointer");
    if (bytes != kBlob.total * sizeof(float)) return h->fail(CID_ERR_SHAPE, "cid_import_packed: size != cid_packed_weights_bytes()");
    std::memcpy(h->staging.data(), host_in, bytes);
    std::memset(h->have, 1, sizeof(h->have));
    return CID_OK;
}

int cid_attach_weights(cid_handle_t h, const void* device_blob) {
    if (!h) return CID_ERR_INVALID;
    if (!device_blob) return h->fail(CID_ERR_INVALID, "cid_attach_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return h->fail(CID_ERR_WORKSPACE, "cid_attach_weights: blob must be 256-byte aligned");
    h->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_out_shape(int H, int W, int* Ho, int* Wo) {
    if (!Ho || !Wo) return CID_ERR_INVALID;
    if (H < 4 || W < 4) return CID_ERR_SHAPE;
    *Ho = 4 * (H / 4);
    *Wo = 4 * (W / 4);
    return CID_OK;
}

int cid_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    Dims d;
    if (shape_error(N, H, W, d)) return CID_ERR_SHAPE;
    *bytes = make_plan(d).total_bytes;
    return CID_OK;
}

int cid_forward(cid_handle_t h, const float* in, float* out, int N, int H, int W, void* ws, size_t ws_bytes, void* stream) {
    return cid_forward_ex(h, in, CID_FMT_F32_NCHW, out, CID_FMT_F32_NCHW, N, H, W, ws, ws_bytes, stream);
}

int cid_forward_ex(cid_handle_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W,
                   void* ws, size_t ws_bytes, void* stream) {
    return run_forward(h, in, in_fmt, out, out_fmt, N, H, W, ws, ws_bytes, static_cast<hipStream_t>(stream));
}

int cid_forward_padded(cid_handle_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W,
                       int pad_left, int pad_top, int pad_right, int pad_bottom, void* ws, size_t ws_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (pad_left < 0 || pad_top < 0 || pad_right < 0 || pad_bottom < 0 || H < 1 || W < 1 || pad_left > 4096 || pad_top > 4096 || pad_right > 4096 || pad_bottom > 4096)
        return h->fail(CID_ERR_INVALID, "cid_forward_padded: paddings must lie in [0, 4096] and the image must not be empty");
    const long long Hp = (long long)H + pad_top + pad_bottom, Wp = (long long)W + pad_left + pad_right;
    if (Hp > 0x7fffffff || Wp > 0x7fffffff) return h->fail(CID_ERR_SHAPE, "cid_forward_padded: padded size overflows");
    int Ho = 0, Wo = 0;
    if (cid_out_shape((int)Hp, (int)Wp, &Ho, &Wo) != CID_OK) return h->fail(CID_ERR_SHAPE, "cid_forward_padded: padded image smaller than 4x4 (output size is too small)");
    // the reference crops [top, top + H) x [left, left + W) out of the network's output (app.py:474-480): that window must exist
    if (pad_top + H > Ho || pad_left + W > Wo) {
        char m[256];
        std::snprintf(m, sizeof m, "cid_forward_padded: the crop window [%d+%d, %d+%d] does not fit the network output %dx%d of the padded image %lldx%lld "
                                   "(pad to a multiple of 4, app.py:276-281)", pad_top, H, pad_left, W, Ho, Wo, Hp, Wp);
        return h->fail(CID_ERR_SHAPE, m);
    }
    const Window src{pad_top, pad_left, H, W}, crop{pad_top, pad_left, H, W};
    return run_forward(h, in, in_fmt, out, out_fmt, N, (int)Hp, (int)Wp, ws, ws_bytes, static_cast<hipStream_t>(stream), nullptr, &src, &crop);
}

int cid_view_u8(const float* in_nchw, void* out_u8_nhwc, int N, int H, int W, void* stream) {
    if (!in_nchw || !out_u8_nhwc || N < 1 || H < 1 || W < 1) return CID_ERR_INVALID;
    const size_t plane = (size_t)H * W, pixels = plane * N;
    if ((pixels + THREADS - 1) / THREADS > 0x7fffffffull) return CID_ERR_SHAPE;
    hipLaunchKernelGGL(k_view_u8, dim3((unsigned)((pixels + THREADS - 1) / THREADS)), dim3(THREADS), 0, static_cast<hipStream_t>(stream),
                       in_nchw, static_cast<unsigned char*>(out_u8_nhwc), plane, pixels);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

int cid_debug_winograd_workgroups_per_cu(int k) {
    const int prev = g_wino42_wg_per_cu;
    if (k >= 0) g_wino42_wg_per_cu = k > 2 ? 2 : k;   // two is what the kernel's LDS use (75 KiB) admits
    return prev;
}
int cid_debug_winograd_column_block_per_xcd(int mask) {
    const int prev = g_wino42_xnb;
    if (mask >= 0) g_wino42_xnb = mask & 6;
    return prev;
}
int cid_debug_half_workgroups_per_cu(int k) {
    const int prev = g_half_wg_per_cu;
    if (k >= 0) g_half_wg_per_cu = k > 3 ? 3 : k;     // three: 47 KiB of LDS, 168 VGPRs
    return prev;
}

int cid_timing_begin(cid_handle_t h, int max_forwards) {
    if (!h) return CID_ERR_INVALID;
    if (max_forwards < 1 || max_forwards > 4096) return h->fail(CID_ERR_INVALID, "cid_timing_begin: max_forwards out of range");
    if (!h->tev.empty()) return h->fail(CID_ERR_STATE, "cid_timing_begin: timing already armed");
    h->tev.resize((size_t)max_forwards * (NL + 1));
    for (size_t i = 0; i < h->tev.size(); ++i)
        if (hipEventCreate(&h->tev[i]) != hipSuccess) {
            for (size_t j = 0; j < i; ++j) (void)hipEventDestroy(h->tev[j]);
            h->tev.clear();
            return h->fail(CID_ERR_HIP, "cid_timing_begin: hipEventCreate failed");
        }
    h->tev_forwards = max_forwards;
    h->tev_used = 0;
    return CID_OK;
}

int cid_timing_end(cid_handle_t h, void* stream, float* launch_ms_sum, int* forwards) {
    if (!h) return CID_ERR_INVALID;
    if (!launch_ms_sum || !forwards) return h->fail(CID_ERR_INVALID, "cid_timing_end: null pointer");
    if (h->tev.empty()) return h->fail(CID_ERR_STATE, "cid_timing_end: timing not armed");
    int rc = CID_OK;
    if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) rc = h->fail(CID_ERR_HIP, "cid_timing_end: stream sync failed");
    for (int l = 0; l < NL; ++l) launch_ms_sum[l] = 0.f;
    for (int f = 0; rc == CID_OK && f < h->tev_used; ++f)
        for (int l = 0; l < NL; ++l) {
            float ms = 0.f;
            const hipEvent_t* e = h->tev.data() + (size_t)f * (NL + 1);
            if (hipEventElapsedTime(&ms, e[l], e[l + 1]) != hipSuccess) { rc = h->fail(CID_ERR_HIP, "cid_timing_end: hipEventElapsedTime failed"); break; }
            launch_ms_sum[l] += ms;
        }
    *forwards = h->tev_used;
    for (hipEvent_t e : h->tev) (void)hipEventDestroy(e);
    h->tev.clear();
    h->tev_forwards = h->tev_used = 0;
    return rc;
}

int cid_forward_timed(cid_handle_t h, const float* in, float* out, int N, int H, int W, void* ws, size_t ws_bytes,
                      void* stream, float* launch_ms) {
    if (!h) return CID_ERR_INVALID;
    if (!launch_ms) return h->fail(CID_ERR_INVALID, "cid_forward_timed: null launch_ms");
    hipEvent_t ev[NL + 1];
    int made = 0;
    for (; made <= NL; ++made)
        if (hipEventCreate(&ev[made]) != hipSuccess) break;
    int rc = made == NL + 1 ? CID_OK : h->fail(CID_ERR_HIP, "hipEventCreate failed");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rc == CID_OK) rc = run_forward(h, in, CID_FMT_F32_NCHW, out, CID_FMT_F32_NCHW, N, H, W, ws, ws_bytes, s, ev);
    if (rc == CID_OK && hipStreamSynchronize(s) != hipSuccess) rc = h->fail(CID_ERR_HIP, "cid_forward_timed: stream sync failed");
    if (rc == CID_OK)
        for (int l = 0; l < NL; ++l)
            if (hipEventElapsedTime(&launch_ms[l], ev[l], ev[l + 1]) != hipSuccess) rc = h->fail(CID_ERR_HIP, "hipEventElapsedTime failed");
    for (int i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
    return rc;
}

const char* cid_launch_name(int i) { return (i >= 0 && i < NL) ? kLayers[i].name : nullptr; }
const char* cid_launch_kernel(cid_handle_t h, int i) {
    if (i < 0 || i >= NL) return nullptr;
    const Config c = config_of(h);
    return kKernelNames.s[c.dtype][c.algo][c.tail][i].c_str();
}

int cid_set_conv_algo(cid_handle_t h, int algo) {
    if (!h) return CID_ERR_INVALID;
    if (algo != CID_ALGO_DIRECT && algo != CID_ALGO_WINOGRAD64 && algo != CID_ALGO_WINOGRAD42 && algo != CID_ALGO_SPLIT16) return h->fail(CID_ERR_INVALID, "cid_set_conv_algo: unknown algorithm");
    h->algo = algo;
    return CID_OK;
}
int cid_set_tail_algo(cid_handle_t h, int algo) {
    if (!h) return CID_ERR_INVALID;
    if (algo != CID_TAIL_FUSED && algo != CID_TAIL_BANDS && algo != CID_TAIL_TILES) return h->fail(CID_ERR_INVALID, "cid_set_tail_algo: unknown algorithm");
    h->tail_algo = algo;
    return CID_OK;
}
int cid_get_tail_algo(cid_handle_t h, int* algo) {
    if (!h || !algo) return CID_ERR_INVALID;
    *algo = h->tail_algo;
    return CID_OK;
}
int cid_set_compute_dtype(cid_handle_t h, int dtype) {
    if (!h) return CID_ERR_INVALID;
    if (dtype != CID_DTYPE_F32 && dtype != CID_DTYPE_F16) return h->fail(CID_ERR_INVALID, "cid_set_compute_dtype: unknown dtype");
    h->dtype = dtype;
    return CID_OK;
}
int cid_get_compute_dtype(cid_handle_t h, int* dtype) {
    if (!h || !dtype) return CID_ERR_INVALID;
    *dtype = h->dtype;
    return CID_OK;
}
// Testing aid: leave NaN in every byte of every CU's LDS.  LDS is not cleared between kernels, so whatever the forward's
// kernels read from LDS without having written it is NaN afterwards (a zero weight does not hide that: 0 x NaN = NaN).
__global__ void __launch_bounds__(256) k_poison_lds() {
    __shared__ float lds[8192];   // 32 KiB: five of these blocks fit a CU and together cover its 160 KiB
    for (int i = threadIdx.x; i < 8192; i += 256) lds[i] = __builtin_nanf("");
    __syncthreads();
    for (int sl = 0; sl < 8; ++sl) __builtin_amdgcn_s_sleep(127);   // stay resident while the CU's other slots fill up
    const float v = lds[threadIdx.x];
    asm volatile("" ::"v"(v));
}
int cid_debug_poison_lds(void* stream) {
    hipLaunchKernelGGL(k_poison_lds, dim3(256 * 5 * 4), dim3(256), 0, static_cast<hipStream_t>(stream));
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

int cid_get_conv_algo(cid_handle_t h, int* algo) {
    if (!h || !algo) return CID_ERR_INVALID;
    *algo = h->algo;
    return CID_OK;
}

// ---- where the reference module's stage outputs live in the arena (tests: per-stage parity) ----
int cid_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* pixel_stride, int* channel_offset) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !pixel_stride || !channel_offset) return CID_ERR_INVALID;
    Dims d;
    if (shape_error(N, H, W, d)) return CID_ERR_SHAPE;
    const Plan p = make_plan(d);
    struct Row { const char* name; Buf buf; int c, hs, ws, ps, coff; };
    const Row rows[] = {
        {"down1", CAT1, 64, d.Hu1, d.Wu1, 128, 64},      // e1, top-left crop Hu1 x Wu1 of H x W       app.py:81,97-100
        {"pool1", P1, 64, d.H1, d.W1, 64, 0},            //                                            app.py:82
        {"down2", CAT2, 128, d.Hu2, d.Wu2, 256, 128},    // e2, top-left crop Hu2 x Wu2 of H1 x W1     app.py:84,90-93
        {"pool2", P2, 128, d.H2, d.W2, 128, 0},          //                                            app.py:85
        {"bottleneck", BT, 256, d.H2, d.W2, 256, 0},     //                                            app.py:87
        {"up2", CAT2, 128, d.Hu2, d.Wu2, 256, 0},        //                                            app.py:89
        {"upconv2", D2, 128, d.Hu2, d.Wu2, 128, 0},      //                                            app.py:94
        {"up1", CAT1, 64, d.Hu1, d.Wu1, 128, 0},         //                                            app.py:96
        {"upconv1.0", T4, 64, d.Hu1, d.Wu1, 64, 0},      // after its ReLU (app.py:75-76); with CID_TAIL_FUSED the region holds
                                                         // the z planes instead (include/cid.h)
        // the first convolution of each two-conv block, after its ReLU (app.py:43-44,51-52,59-60,67-68): every launch writes a
        // region of its own (enum Buf), so these are still intact after the forward
        {"down1.0", T0, 64, d.H, d.W, 64, 0},
        {"down2.0", T1, 128, d.H1, d.W1, 128, 0},
        {"bottleneck.0", T2, 256, d.H2, d.W2, 256, 0},
        {"upconv2.0", T3, 128, d.Hu2, d.Wu2, 128, 0},
    };
    for (const Row& r : rows)
        if (std::strcmp(stage, r.name) == 0) {
            *offset_bytes = p.off[r.buf] * sizeof(float);
            *C = r.c; *Hs = r.hs; *Ws = r.ws; *pixel_stride = r.ps; *channel_offset = r.coff;
            return CID_OK;
        }
    return CID_ERR_KEY;
}

// ---- multi-GPU: the one collective of the job, without PyTorch in it ----
// RCCL is bound at run time from the process (the library that created the caller's communicator), not linked: libcid.so
// loads on a box without RCCL, and a host that already has an RCCL (PyTorch ships its own librccl.so.1) keeps exactly one.
}  // extern "C"
namespace {
struct Rccl {
    typedef int (*GetUniqueId)(void*);
    typedef int (*CommInitRank)(void**, int, ncclUniqueIdBytes, int);
    typedef int (*CommDestroy)(void*);
    typedef int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t);
    typedef const char* (*GetErrorString)(int);
    typedef int (*CommCount)(void*, int*);
    GetUniqueId get_unique_id = nullptr; CommInitRank comm_init_rank = nullptr; CommDestroy comm_destroy = nullptr;
    Broadcast broadcast = nullptr; GetErrorString error_string = nullptr; CommCount comm_count = nullptr;
    std::string why;
    bool ok = false;
};
const Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);          // the copy this process already uses
        if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) lib = dlopen("/opt/rocm/lib/librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) { x.why = std::string("librccl.so.1 not found: ") + dlerror(); return x; }
        x.get_unique_id = (Rccl::GetUniqueId)dlsym(lib, "ncclGetUniqueId");
        x.comm_init_rank = (Rccl::CommInitRank)dlsym(lib, "ncclCommInitRank");
        x.comm_destroy = (Rccl::CommDestroy)dlsym(lib, "ncclCommDestroy");
        x.broadcast = (Rccl::Broadcast)dlsym(lib, "ncclBroadcast");
        x.error_string = (Rccl::GetErrorString)dlsym(lib, "ncclGetErrorString");
        x.comm_count = (Rccl::CommCount)dlsym(lib, "ncclCommCount");   // optional: only cid_comm_count needs it
        x.ok = x.get_unique_id && x.comm_init_rank && x.comm_destroy && x.broadcast && x.error_string;
        if (!x.ok) x.why = "librccl.so.1 lacks ncclGetUniqueId/ncclCommInitRank/ncclCommDestroy/ncclBroadcast";
        return x;
    }();
    return r;
}
int rccl_fail(cid_handle_t h, const char* what, int rc) {
    return h->fail(CID_ERR_HIP, std::string(what) + ": " + (rccl().error_string ? rccl().error_string(rc) : "RCCL error"));
}
}  // namespace
extern "C" {

int cid_comm_available(void) { return rccl().ok ? 1 : 0; }
int cid_comm_unique_id(void* id128) {
    if (!id128) return CID_ERR_INVALID;
    if (!rccl().ok) return CID_ERR_STATE;
    return rccl().get_unique_id(id128) == 0 ? CID_OK : CID_ERR_HIP;
}
int cid_comm_init_rank(void** comm, int nranks, const void* id128, int rank) {
    if (!comm || !id128 || nranks < 1 || rank < 0 || rank >= nranks) return CID_ERR_INVALID;
    if (!rccl().ok) return CID_ERR_STATE;
    ncclUniqueIdBytes id;
    std::memcpy(&id, id128, sizeof id);
    return rccl().comm_init_rank(comm, nranks, id, rank) == 0 ? CID_OK : CID_ERR_HIP;
}
int cid_comm_destroy(void* comm) {
    if (!comm) return CID_ERR_INVALID;
    if (!rccl().ok) return CID_ERR_STATE;
    return rccl().comm_destroy(comm) == 0 ? CID_OK : CID_ERR_HIP;
}
int cid_comm_count(void* comm, int* nranks) {
    if (!comm || !nranks) return CID_ERR_INVALID;
    if (!rccl().ok || !rccl().comm_count) return CID_ERR_STATE;
    return rccl().comm_count(comm, nranks) == 0 ? CID_OK : CID_ERR_HIP;
}

int cid_broadcast_weights(cid_handle_t h, void* comm, int root, int rank, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!comm || root < 0 || rank < 0) return h->fail(CID_ERR_INVALID, "cid_broadcast_weights: null communicator or negative rank");
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, "cid_broadcast_weights: no device blob attached (root: cid_upload_weights; receivers: cid_attach_weights on an allocated buffer)");
    if (!rccl().ok) return h->fail(CID_ERR_STATE, "cid_broadcast_weights: " + rccl().why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    void* blob = const_cast<float*>(h->dev_blob);
    const size_t bytes = kBlob.total * sizeof(float);
    const int rc = rccl().broadcast(blob, blob, bytes, /*ncclUint8*/ 1, root, comm, s);   // in place: one 26 MB message, root -> everyone
    if (rc != 0) return rccl_fail(h, "ncclBroadcast", rc);
    if (rank != root) {   // receivers: refresh the host staging copy, so cid_get_weight / state_dict() return what the kernels use
        hipError_t e = hipMemcpyAsync(h->staging.data(), blob, bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return h->fail(CID_ERR_HIP, std::string("cid_broadcast_weights: ") + hipGetErrorString(e));
        std::memset(h->have, 1, sizeof(h->have));
    }
    return CID_OK;
}

int cid_launch_work(int i, int N, int H, int W, double* flops, double* bytes) {
    if (i < 0 || i >= NL || !flops || !bytes) return CID_ERR_INVALID;
    Dims d;
    if (!make_dims(N, H, W, d)) return CID_ERR_SHAPE;
    // output pixels (conv) / input pixels (convT) per image, as the reference evaluates each layer
    const double s0 = (double)d.H * d.W, s1 = (double)d.H1 * d.W1, s2 = (double)d.H2 * d.W2;
    const double su2 = (double)d.Hu2 * d.Wu2, su1 = (double)d.Hu1 * d.Wu1;
    const double pix[NL] = {s0, s0, s1, s1, s2, s2, s2, su2, su2, su2, su1, su1};
    const LayerDef& L = kLayers[i];
    const double taps = L.kind == CONVT ? 4 : 9;
    *flops = 2.0 * L.cin * L.cout * taps * pix[i] * N;
    const double out_pix = L.kind == CONVT ? 4 * pix[i] : pix[i];
    *bytes = 4.0 * (N * (pix[i] * L.cin + out_pix * L.cout) + (double)ref_weight_count(L) + L.cout);
    return CID_OK;
}

// The same per LAUNCH under the handle's configuration.  It differs from the per-layer figures (a) on launches 1 and 3, which write the pooled
// tensor beside their own output (the reference's MaxPool2d modules are fused into them), and (b) when the last layer's
// channel contraction is fused into upconv1[0]'s launch (CID_TAIL_FUSED): launch 10 then carries the FLOPs of both layers and
// writes 27 z planes instead of 64 channels; launch 11 is the shifted sum (no multiply-adds) over those planes.
int cid_launch_work_ex(cid_handle_t h, int i, int N, int H, int W, double* flops, double* bytes) {
    const int rc = cid_launch_work(i, N, H, W, flops, bytes);
    if (rc != CID_OK) return rc;
    Dims d;
    make_dims(N, H, W, d);
    // launches 1 and 3 (down1[2], down2[2]) also write the 2x2-pooled tensor from their epilogue (pool1 / pool2, app.py:48,56: SURVEY 8a rows a3 / a6 —
    // the pools' reads are what the fusion removes, their writes remain): in every configuration of the handle
    if (i == 1) *bytes += 4.0 * N * (double)d.H1 * d.W1 * kLayers[1].cout;
    if (i == 3) *bytes += 4.0 * N * (double)d.H2 * d.W2 * kLayers[3].cout;
    const Kern tail = select_kernel(config_of(h), 11);
    if ((tail != Kern::TAIL_Z && tail != Kern::TAIL_ZH) || i < 10) return rc;
    const double px = (double)N * d.Hu1 * d.Wu1;
    double f11, b11;
    cid_launch_work(11, N, H, W, &f11, &b11);
    // z elements per pixel: 27 fp32 planes; on the fp16-storage path 7 groups x 4 halfs (27 rows and a pad), counted here in
    // fp32-sized elements like every other activation of that path (bench.py halves the bytes between the first and the last tensor)
    const double zc = tail == Kern::TAIL_ZH ? 28 : 27;
    if (i == 10) {
        *flops += f11;
        *bytes += 4.0 * px * (zc - 64) + 4.0 * ref_weight_count(kLayers[11]);
    } else {
        *flops = 0.0;
        *bytes = 4.0 * (px * (zc + 3) + 3);
    }
    return CID_OK;
}

}  // extern "C"

// ---- the other families, one host file each; their place here fixes the order in which kernel templates are first instantiated ----
#include "api/quality.h"          // cid_quality
#include "api/noise.h"            // cid_add_noise
#include "api/resize.h"           // cid_resize_*
#include "api/disc_forward.h"     // the BatchNorm discriminators' shared description; cid_disc_*: weights, forward
#include "api/disc_backward.h"    // their shared backward side; cid_disc_*: saved forward, backward, device pack, masks, losses
#include "api/srgan_disc.h"       // cid_srd_*: the SRGAN trainer's discriminator, forward and losses
#include "api/srgan_disc_backward.h"   // cid_srd_*: saved forward, backward, device pack, masks
#include "api/esrgan_disc.h"      // cid_esd_*: the ESRGAN trainer's discriminator, weights, forward plan and losses
#include "api/esrgan_disc_backward.h"  // cid_esd_*: forward, saved forward, backward, device pack
#include "api/adam.h"             // cid_adam_step

// ---- the generator's backward pass (gen_bwd_kernels.h) ----
namespace {

// Workspace of one cid_backward call: the gradients of the activations (NHWC fp32, finished dz where a ReLU follows) and the
// partial tiles of the weight gradients.  G4 (dz of upconv1.0) is dead before GT0 (dz of down1.0) is written and GD2 before GT1.
struct GenBwdPlan {
    size_t dz16, G4, dcat1, gd2, gt3, dcat2, gbt, gt2, dp2, dp1, part, part_b, part27, part27_b, total;
    int splits[NL];       // range split of each GEMM-shaped layer's weight gradient
    int w27_strips, w27_splits;
};

// The weight-gradient GEMM of layer l: row operand channels R, column operand channels C, taps, and the row operand's size.
struct GenWg { int R, C, taps, Hr, Wr; };
GenWg gen_wg(int l, const Dims& d) {
    const LayerDef& L = kLayers[l];
    const int res = (l == 1 || l == 10) ? 0 : (l == 4 || l == 5 || l == 6) ? 2 : 1;   // resolution of the row operand
    const int Hr = res == 0 ? d.H : res == 1 ? d.H1 : d.H2, Wr = res == 0 ? d.W : res == 1 ? d.W1 : d.W2;
    if (L.kind == CONVT) return {L.cin, L.cout, 4, Hr, Wr};
    return {L.cout, L.cin, 9, Hr, Wr};
}
int gen_wg_tiles_x(const GenWg& g) { return cdiv(g.Wr, G_TW); }
int gen_wg_tiles(const GenWg& g) { return cdiv(g.Hr, G_WG_TH) * gen_wg_tiles_x(g); }

void gen_bwd_plan(const Dims& d, GenBwdPlan& q) {
    const size_t n = (size_t)d.N, f = sizeof(float);
    const size_t s0 = n * d.H * d.W, s1 = n * d.H1 * d.W1, s2 = n * d.H2 * d.W2;
    size_t part = 0, part_b = 0;
    for (int l = 1; l <= 10; ++l) {
        const GenWg g = gen_wg(l, d);
        const long long items = (long long)d.N * gen_wg_tiles(g);
        const int groups = (g.C / 16) * std::max(1, g.R / 128);
        q.splits[l] = (int)std::min<long long>(items, std::max(1, 1024 / groups));
        part = std::max(part, (size_t)q.splits[l] * g.R * g.C * g.taps * f);
        part_b = std::max(part_b, (size_t)q.splits[l] * std::max(g.R, g.C) * sizeof(double));
    }
    q.splits[0] = q.splits[11] = 0;
    q.w27_strips = (int)(((long long)d.H * d.W + 63) / 64);
    q.w27_splits = (int)std::min<long long>((long long)d.N * q.w27_strips, 1024);
    size_t at = 0;
    q.dz16 = take(at, s0 * 3 * f);
    q.G4 = take(at, s0 * 64 * f);
    q.dcat1 = take(at, s0 * 128 * f);
    q.gd2 = take(at, s1 * 128 * f);
    q.gt3 = take(at, s1 * 128 * f);
    q.dcat2 = take(at, s1 * 256 * f);
    q.gbt = take(at, s2 * 256 * f);
    q.gt2 = take(at, s2 * 256 * f);
    q.dp2 = take(at, s2 * 128 * f);
    q.dp1 = take(at, s1 * 64 * f);
    q.part = take(at, part);
    q.part_b = take(at, part_b);
    q.part27 = take(at, (size_t)q.w27_splits * 64 * 28 * sizeof(double));
    q.part27_b = take(at, (size_t)q.w27_splits * 3 * sizeof(double));
    q.total = at;
}

// Why an [N,3,H,W] batch cannot be differentiated, or nullptr.
const char* gen_bwd_shape_error(int N, int H, int W, Dims& d) {
    if (const char* why = shape_error(N, H, W, d)) return why;
    if (H % 4 || W % 4)
        return "H and W must be multiples of 4 for the differentiable forward (for other sizes the skip tensors are stored only over the crop, "
               "so the max-pool routing outside it cannot be recovered)";
    return nullptr;
}

struct GenView { const float* p; int ps, coff; };

template <int CD, int CXB, int TAPS>
hipError_t gen_dgrad_launch(GenDgradArgs a, int N, hipStream_t s) {
    using G = GenDgradGeom<CXB, TAPS>;
    a.tiles_x = cdiv(a.W, G_TW);
    a.tiles = cdiv(a.H, G::TH) * a.tiles_x;
    (void)for_each_launch(N, [&](int n0, int n) {
        a.n0 = n0;
        const dim3 grid((unsigned)(a.tiles * (a.CX / CXB)), (unsigned)n);
        hipLaunchKernelGGL((k_gen_dgrad<CD, CXB, TAPS>), grid, dim3(G_THREADS), 0, s, a);
    });
    return hipGetLastError();
}

// The data gradient of GEMM-shaped layer l (1 ... 10).
hipError_t gen_dgrad(int l, const GenDgradArgs& a, int N, hipStream_t s) {
    switch (l) {
        case 10: return gen_dgrad_launch<64, 128, 9>(a, N, s);
        case 9: return gen_dgrad_launch<64, 128, 4>(a, N, s);
        case 8: case 7: case 3: return gen_dgrad_launch<128, 128, 9>(a, N, s);
        case 6: return gen_dgrad_launch<128, 128, 4>(a, N, s);
        case 5: case 4: return gen_dgrad_launch<256, 128, 9>(a, N, s);
        case 2: return gen_dgrad_launch<128, 64, 9>(a, N, s);
        case 1: return gen_dgrad_launch<64, 64, 9>(a, N, s);
        default: return hipErrorInvalidValue;
    }
}

hipError_t gen_wgrad(const GenWg& g, GenWgradArgs a, float* dw, float* db, hipStream_t s) {
    a.Hr = g.Hr; a.Wr = g.Wr; a.R = g.R; a.C = g.C;
    a.tiles_x = gen_wg_tiles_x(g); a.tiles = gen_wg_tiles(g);
    const bool convt = g.taps == 4;
    const int crb = g.R >= 128 ? 128 : 64;
    const dim3 grid((unsigned)a.splits, (unsigned)(g.C / 16), (unsigned)(g.R / crb));
    if (convt) hipLaunchKernelGGL((k_gen_wgrad<128, true>), grid, dim3(G_THREADS), 0, s, a);
    else if (crb == 128) hipLaunchKernelGGL((k_gen_wgrad<128, false>), grid, dim3(G_THREADS), 0, s, a);
    else hipLaunchKernelGGL((k_gen_wgrad<64, false>), grid, dim3(G_THREADS), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int nb = convt ? g.C : g.R;
    const GenWgradReduceArgs r{a.part, a.part_b, dw, db, a.splits, g.R, g.C, g.taps, nb};
    hipLaunchKernelGGL(k_gen_wgrad_reduce, dim3((unsigned)cdiv(g.R * g.C * g.taps + nb, G_THREADS)), dim3(G_THREADS), 0, s, r);
    return hipGetLastError();
}

}  // namespace

extern "C" {

int cid_saved_bytes(int N, int H, int W, size_t* bytes) { return cid_workspace_bytes(N, H, W, bytes); }

int cid_forward_saved(cid_handle_t h, const float* in, float* out, int N, int H, int W, void* saved, size_t saved_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_forward_saved", stream);
    if (!in || !out || !saved) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (h->dtype != CID_DTYPE_F32) return cx.fail(CID_ERR_STATE, "the differentiable forward needs compute dtype CID_DTYPE_F32");
    Dims d;
    if (const char* why = gen_bwd_shape_error(N, H, W, d)) {
        char m[384];
        std::snprintf(m, sizeof m, "cid_forward_saved: input [%d,3,%d,%d] not accepted: %s", N, H, W, why);
        return h->fail(CID_ERR_SHAPE, m);
    }
    if (const int rc = cx.room(saved, saved_bytes, make_plan(d).total_bytes, "cid_saved_bytes", "saved buffer")) return rc;
    if (!h->dev_blob) return cx.fail(CID_ERR_STATE, "no device weights attached (call cid_upload_weights or cid_attach_weights)");
    // the last layer as a launch of its own: the fused form never stores upconv1.0, which the backward pass reads
    const Config cfg{CID_DTYPE_F32, h->algo, CID_TAIL_TILES};
    return run_forward(h, in, CID_FMT_F32_NCHW, out, CID_FMT_F32_NCHW, N, H, W, saved, saved_bytes, static_cast<hipStream_t>(stream), nullptr,
                       nullptr, nullptr, &cfg);
}

int cid_backward_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    Dims d;
    if (gen_bwd_shape_error(N, H, W, d)) return CID_ERR_SHAPE;
    GenBwdPlan q;
    gen_bwd_plan(d, q);
    *bytes = q.total;
    return CID_OK;
}

int cid_backward(cid_handle_t h, const float* in, const float* out, const float* grad_out, int N, int H, int W, const void* saved,
                 size_t saved_bytes, const cid_grads* g, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const Call cx(h, "cid_backward", stream);
    if (!in || !out || !grad_out || !saved || !g || !workspace) return cx.fail(CID_ERR_INVALID, "null pointer");
    if (h->dtype != CID_DTYPE_F32) return cx.fail(CID_ERR_STATE, "the backward pass needs compute dtype CID_DTYPE_F32");
    bool misaligned = ((uintptr_t)in & 3) || ((uintptr_t)out & 3) || ((uintptr_t)grad_out & 3) || ((uintptr_t)g->input & 3);
    for (int l = 0; l < NL; ++l) misaligned = misaligned || ((uintptr_t)g->w[l] & 3) || ((uintptr_t)g->b[l] & 3);
    if (misaligned) return cx.fail(CID_ERR_INVALID, "misaligned fp32 pointer");
    Dims d;
    if (const char* why = gen_bwd_shape_error(N, H, W, d)) {
        char m[384];
        std::snprintf(m, sizeof m, "cid_backward: input [%d,3,%d,%d] not accepted: %s", N, H, W, why);
        return h->fail(CID_ERR_SHAPE, m);
    }
    const Plan p = make_plan(d);
    if (const int rc = cx.room(saved, saved_bytes, p.total_bytes, "cid_saved_bytes", "saved buffer")) return rc;
    GenBwdPlan q;
    gen_bwd_plan(d, q);
    if (const int rc = cx.room(workspace, workspace_bytes, q.total, "cid_backward_workspace_bytes")) return rc;
    if (!h->dev_blob) return cx.fail(CID_ERR_STATE, "no device weights attached (call cid_upload_weights or cid_attach_weights)");

    const hipStream_t s = cx.s;
    const float* sv = static_cast<const float*>(saved);
    const float* B[NBUF];
    for (int b = 0; b < NBUF; ++b) B[b] = sv + p.off[b];
    char* ws = static_cast<char*>(workspace);
    const auto wsf = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    float* dz16 = wsf(q.dz16);
    float *G4 = wsf(q.G4), *dcat1 = wsf(q.dcat1), *gd2 = wsf(q.gd2), *gt3 = wsf(q.gt3), *dcat2 = wsf(q.dcat2), *gbt = wsf(q.gbt);
    float *gt2 = wsf(q.gt2), *dp2 = wsf(q.dp2), *dp1 = wsf(q.dp1), *gt0 = G4, *gt1 = gd2;
    float* part = wsf(q.part);
    double* part_b = reinterpret_cast<double*>(ws + q.part_b);
    double* part27 = reinterpret_cast<double*>(ws + q.part27);
    double* part27_b = reinterpret_cast<double*>(ws + q.part27_b);
    const float* blob = h->dev_blob;

    // below[l]: the input gradient or a parameter gradient of a layer before l is asked for, so layer l's data gradient is needed
    bool need[NL], below[NL + 1];
    below[0] = g->input != nullptr;
    for (int l = 0; l < NL; ++l) {
        need[l] = g->w[l] || g->b[l];
        below[l + 1] = below[l] || need[l];
    }
    if (!below[NL]) return CID_OK;

    // Per GEMM-shaped layer l: the layer's input (column operand of a convolution's weight gradient, the stored activation), its dz
    // (the gradient of its pre-activation output) and where its data gradient goes, with the activation whose mask finishes it.
    struct Row { GenView in; GenView dz; float* dout; int out_ps; const float* act; int act_ps; int Ho, Wo; };
    const Row rows[NL] = {
        {},
        /* 1 down1.2     */ {{B[T0], 64, 0}, {dcat1, 128, 64}, gt0, 64, B[T0], 64, d.H, d.W},
        /* 2 down2.0     */ {{B[P1], 64, 0}, {gt1, 128, 0}, dp1, 64, nullptr, 0, d.H1, d.W1},
        /* 3 down2.2     */ {{B[T1], 128, 0}, {dcat2, 256, 128}, gt1, 128, B[T1], 128, d.H1, d.W1},
        /* 4 bottleneck.0*/ {{B[P2], 128, 0}, {gt2, 256, 0}, dp2, 128, nullptr, 0, d.H2, d.W2},
        /* 5 bottleneck.2*/ {{B[T2], 256, 0}, {gbt, 256, 0}, gt2, 256, B[T2], 256, d.H2, d.W2},
        /* 6 up2         */ {{B[BT], 256, 0}, {dcat2, 256, 0}, gbt, 256, B[BT], 256, d.H2, d.W2},
        /* 7 upconv2.0   */ {{B[CAT2], 256, 0}, {gt3, 128, 0}, dcat2, 256, nullptr, 0, d.H1, d.W1},
        /* 8 upconv2.2   */ {{B[T3], 128, 0}, {gd2, 128, 0}, gt3, 128, B[T3], 128, d.H1, d.W1},
        /* 9 up1         */ {{B[D2], 128, 0}, {dcat1, 128, 0}, gd2, 128, B[D2], 128, d.H1, d.W1},
        /*10 upconv1.0   */ {{B[CAT1], 128, 0}, {G4, 64, 0}, dcat1, 128, nullptr, 0, d.H, d.W},
        {},
    };

    // upconv1.2 (+ tanh)
    {
        const long long total = (long long)N * 3 * H * W;
        hipLaunchKernelGGL(k_gen_dz16, dim3((unsigned)((total + G_THREADS - 1) / G_THREADS)), dim3(G_THREADS), 0, s, grad_out, out, dz16, total);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("dz16");
    }
    if (need[11]) {
        const GenWgrad27Args a{dz16, B[T4], 64, 0, part27, part27_b, (long long)N * q.w27_strips, q.w27_splits, q.w27_strips, H, W};
        hipLaunchKernelGGL(k_gen_wgrad27<true>, dim3((unsigned)q.w27_splits), dim3(G_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("upconv1.2 weight gradient");
        const GenWgrad27ReduceArgs r{part27, part27_b, g->w[11], g->b[11], q.w27_splits};
        hipLaunchKernelGGL(k_gen_wgrad27_reduce<true>, dim3((unsigned)cdiv(64 * 28 + 3, G_THREADS)), dim3(G_THREADS), 0, s, r);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("upconv1.2 weight gradient reduce");
    }
    if (!below[11]) return CID_OK;
    {
        const long long pixels = (long long)N * H * W;
        const GenDgradTailArgs a{dz16, blob + kBlob.raw_w_off[11], B[T4], G4, pixels, H, W};
        hipLaunchKernelGGL(k_gen_dgrad_tail, dim3((unsigned)((pixels + 63) / 64)), dim3(G_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("upconv1.2 data gradient");
    }

    for (int l = 10; l >= 1; --l) {
        const Row& r = rows[l];
        const bool convt = kLayers[l].kind == CONVT;
        if (need[l]) {
            const GenWg wg = gen_wg(l, d);
            GenWgradArgs a{};
            // row operand: dz of a convolution, the input of a transposed convolution; column operand: the other one
            const GenView& ro = convt ? r.in : r.dz;
            const GenView& co = convt ? r.dz : r.in;
            a.r = ro.p; a.r_ps = ro.ps; a.r_coff = ro.coff;
            a.c = co.p; a.c_ps = co.ps; a.c_coff = co.coff;
            a.part = part; a.part_b = part_b;
            a.items = (long long)N * gen_wg_tiles(wg);
            a.splits = q.splits[l];
            if (gen_wgrad(wg, a, g->w[l], g->b[l], s) != hipSuccess) return cx.hip(std::string(kLayers[l].name) + " weight gradient");
        }
        if (!below[l]) return CID_OK;
        GenDgradArgs a{};
        a.dz = r.dz.p; a.dz_ps = r.dz.ps; a.dz_coff = r.dz.coff;
        a.w = blob + kBlob.raw_w_off[l];
        a.act = r.act; a.act_ps = r.act_ps; a.act_coff = 0;
        a.out = r.dout; a.out_ps = r.out_ps; a.out_coff = 0;
        a.H = r.Ho; a.W = r.Wo; a.CX = kLayers[l].cin;
        if (gen_dgrad(l, a, N, s) != hipSuccess) return cx.hip(std::string(kLayers[l].name) + " data gradient");
        if (l == 4 || l == 2) {   // the pooled tensor's gradient is complete: finish dz of the skip tensor under it
            GenPoolBwdArgs pa{};
            const int C = l == 4 ? 128 : 64;
            pa.e = l == 4 ? B[CAT2] : B[CAT1]; pa.e_ps = 2 * C; pa.e_coff = C;
            pa.dp = l == 4 ? dp2 : dp1;
            pa.io = l == 4 ? dcat2 : dcat1; pa.io_ps = 2 * C; pa.io_coff = C;
            pa.Hp = r.Ho; pa.Wp = r.Wo;
            pa.total = (long long)N * r.Ho * r.Wo * (C / 4);
            const long long blocks = (pa.total + G_THREADS - 1) / G_THREADS;
            if (blocks > 0x7fffffffLL) return cx.fail(CID_ERR_SHAPE, "batch too large for one call");
            if (l == 4) hipLaunchKernelGGL(k_gen_pool_bwd<128>, dim3((unsigned)blocks), dim3(G_THREADS), 0, s, pa);
            else hipLaunchKernelGGL(k_gen_pool_bwd<64>, dim3((unsigned)blocks), dim3(G_THREADS), 0, s, pa);
            if (hipPeekAtLastError() != hipSuccess) return cx.hip("max-pool gradient");
        }
    }

    // down1.0
    if (need[0]) {
        const GenWgrad27Args a{in, gt0, 64, 0, part27, part27_b, (long long)N * q.w27_strips, q.w27_splits, q.w27_strips, H, W};
        hipLaunchKernelGGL(k_gen_wgrad27<false>, dim3((unsigned)q.w27_splits), dim3(G_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("down1.0 weight gradient");
        const GenWgrad27ReduceArgs r{part27, part27_b, g->w[0], g->b[0], q.w27_splits};
        hipLaunchKernelGGL(k_gen_wgrad27_reduce<false>, dim3((unsigned)cdiv(64 * 28, G_THREADS)), dim3(G_THREADS), 0, s, r);
        if (hipPeekAtLastError() != hipSuccess) return cx.hip("down1.0 weight gradient reduce");
    }
    if (g->input) {
        if (const int rc = cx.launches(N, "down1.0 data gradient", [&](int n0, int n) {
            const GenDgradHeadArgs a{gt0, blob + kBlob.raw_w_off[0], g->input, H, W, n0};
            const dim3 grid((unsigned)(((long long)H * W + G_THREADS - 1) / G_THREADS), (unsigned)n);
            hipLaunchKernelGGL(k_gen_dgrad_head, grid, dim3(G_THREADS), 0, s, a);
        })) return rc;
    }
    return CID_OK;
}

}  // extern "C"

#include "api/esrgan.h"           // cid_esr_*
#include "api/srgan.h"            // cid_sr_*
#include "api/srgan_train.h"      // cid_sr_*: the train-mode forward (batch-statistics BatchNorm)
#include "api/esrgan_train.h"     // cid_esr_*: the train-mode forward (batch-statistics BatchNorm under the blocks' skips)
#include "api/srgan_backward.h"   // cid_sr_*: saved train forward, backward, masks
#include "api/esrgan_backward.h"  // cid_esr_*: saved train forward, backward, device pack, masks
#include "api/cgan.h"             // cid_cg_*
#include "api/lpips.h"            // cid_lpips_*
#include "api/vgg.h"              // cid_vgg_*
