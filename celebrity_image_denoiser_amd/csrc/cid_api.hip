// cid_api.hip — the C ABI of include/cid.h: weight repacking, workspace planning and the launch
// sequence of one forward.  Host code; the device kernels are in conv_kernels.h.
//
// Layer table = the reference module's declaration order, backend/app.py:42-78.
#include "../../include/cid.h"
#include "conv_kernels.h"
#include "wino64_kernels.h"
#include "wino42_kernels.h"
#include "conv_kernels_f16.h"
#include "quality_kernels.h"
#include "noise_kernels.h"
#include "disc_kernels.h"
#include "disc_bwd_kernels.h"
#include "gen_bwd_kernels.h"
#include "gen_pack_kernels.h"
#include "optim_kernels.h"
#include "resize_kernels.h"
#include "esrgan_kernels.h"
#include "srgan_kernels.h"
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

struct cid_handle_s {
    std::vector<float> staging;        // packed host blob
    bool have[NL][2];
    const float* dev_blob = nullptr;
    std::string err;
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

int fail(cid_handle_t h, int code, const std::string& msg) {
    if (h) h->err = msg;
    return code;
}

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

inline int cdiv(int a, int b) { return (a + b - 1) / b; }

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
    if (!in || !out || !ws) return fail(h, CID_ERR_INVALID, "cid_forward: null pointer");
    if (!h->dev_blob) return fail(h, CID_ERR_STATE, "cid_forward: no device weights attached (call cid_upload_weights or cid_attach_weights)");
    Dims d;
    if (const char* why = shape_error(N, H, W, d)) {
        char m[256];
        std::snprintf(m, sizeof m, "cid_forward: input [%d,3,%d,%d] not accepted: %s", N, H, W, why);
        return fail(h, CID_ERR_SHAPE, m);
    }
    const Plan p = make_plan(d);
    if (ws_bytes < p.total_bytes) return fail(h, CID_ERR_WORKSPACE, "cid_forward: workspace smaller than cid_workspace_bytes()");
    if ((in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) || (out_fmt != CID_FMT_F32_NCHW && out_fmt != CID_FMT_U8_NHWC))
        return fail(h, CID_ERR_INVALID, "cid_forward: unknown tensor format");
    if (((uintptr_t)ws & 255) || ((uintptr_t)h->dev_blob & 255) || (in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)))
        return fail(h, CID_ERR_WORKSPACE, "cid_forward: workspace/weights must be 256-byte aligned, fp32 input 4-byte aligned");
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
            return fail(h, CID_ERR_HIP, std::string("launch '") + kLayers[li].name + "' failed: " + hipGetErrorString(e)); \
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
    if (ev && hipEventRecord(ev[NL], s) != hipSuccess) return fail(h, CID_ERR_HIP, "hipEventRecord failed");
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
    if (!key || !data || !shape) return fail(h, CID_ERR_INVALID, "cid_set_weight: null argument");
    int l, is_bias;
    if (!find_key(key, l, is_bias)) return fail(h, CID_ERR_KEY, std::string("unexpected key '") + key + "' in state_dict");
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
        return fail(h, CID_ERR_SHAPE, m + "]");
    }
    stage_segments(h->staging.data(), 2 * l + is_bias, data);   // every layout of this tensor, the reference-layout copy included
    h->have[l][is_bias] = true;
    return CID_OK;
}

int cid_get_weight(cid_handle_t h, const char* key, float* out, size_t count) {
    if (!h) return CID_ERR_INVALID;
    if (!key || !out) return fail(h, CID_ERR_INVALID, "cid_get_weight: null argument");
    int l, is_bias;
    if (!find_key(key, l, is_bias)) return fail(h, CID_ERR_KEY, std::string("unknown key '") + key + "'");
    const LayerDef& L = kLayers[l];
    const size_t need = is_bias ? (size_t)L.cout : ref_weight_count(L);
    if (count != need) return fail(h, CID_ERR_SHAPE, std::string("cid_get_weight: wrong element count for ") + key);
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
    if (!device_blob) return fail(h, CID_ERR_INVALID, "cid_upload_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return fail(h, CID_ERR_WORKSPACE, "cid_upload_weights: blob must be 256-byte aligned");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(device_blob, h->staging.data(), kBlob.total * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // staging is pageable host memory owned by the handle
    if (e != hipSuccess) return fail(h, CID_ERR_HIP, std::string("cid_upload_weights: ") + hipGetErrorString(e));
    h->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_pack_weights_device(cid_handle_t h, const float* const* dev_params, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!dev_params || !device_blob) return fail(h, CID_ERR_INVALID, "cid_pack_weights_device: null pointer");
    for (int i = 0; i < CID_NUM_PARAMS; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3))
            return fail(h, CID_ERR_INVALID, "cid_pack_weights_device: null or misaligned parameter pointer");
    if ((uintptr_t)device_blob & 255) return fail(h, CID_ERR_WORKSPACE, "cid_pack_weights_device: blob must be 256-byte aligned");
    const GenPackArgs a = gen_pack_args(dev_params, device_blob);
    hipLaunchKernelGGL(k_gen_pack, dim3((a.nitems + GP_THREADS / 64 - 1) / (GP_THREADS / 64)), dim3(GP_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return fail(h, CID_ERR_HIP, "cid_pack_weights_device: launch failed");
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
    if (!host_out) return fail(h, CID_ERR_INVALID, "cid_export_packed: null pointer");
    if (bytes != kBlob.total * sizeof(float)) return fail(h, CID_ERR_SHAPE, "cid_export_packed: size != cid_packed_weights_bytes()");
    std::memcpy(host_out, h->staging.data(), bytes);
    return CID_OK;
}

int cid_import_packed(cid_handle_t h, const void* host_in, size_t bytes) {
    if (!h) return CID_ERR_INVALID;
    if (!host_in) return fail(h, CID_ERR_INVALID, "cid_import_packed: null pointer");
    if (bytes != kBlob.total * sizeof(float)) return fail(h, CID_ERR_SHAPE, "cid_import_packed: size != cid_packed_weights_bytes()");
    std::memcpy(h->staging.data(), host_in, bytes);
    std::memset(h->have, 1, sizeof(h->have));
    return CID_OK;
}

int cid_attach_weights(cid_handle_t h, const void* device_blob) {
    if (!h) return CID_ERR_INVALID;
    if (!device_blob) return fail(h, CID_ERR_INVALID, "cid_attach_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return fail(h, CID_ERR_WORKSPACE, "cid_attach_weights: blob must be 256-byte aligned");
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
        return fail(h, CID_ERR_INVALID, "cid_forward_padded: paddings must lie in [0, 4096] and the image must not be empty");
    const long long Hp = (long long)H + pad_top + pad_bottom, Wp = (long long)W + pad_left + pad_right;
    if (Hp > 0x7fffffff || Wp > 0x7fffffff) return fail(h, CID_ERR_SHAPE, "cid_forward_padded: padded size overflows");
    int Ho = 0, Wo = 0;
    if (cid_out_shape((int)Hp, (int)Wp, &Ho, &Wo) != CID_OK) return fail(h, CID_ERR_SHAPE, "cid_forward_padded: padded image smaller than 4x4 (output size is too small)");
    // the reference crops [top, top + H) x [left, left + W) out of the network's output (app.py:474-480): that window must exist
    if (pad_top + H > Ho || pad_left + W > Wo) {
        char m[256];
        std::snprintf(m, sizeof m, "cid_forward_padded: the crop window [%d+%d, %d+%d] does not fit the network output %dx%d of the padded image %lldx%lld "
                                   "(pad to a multiple of 4, app.py:276-281)", pad_top, H, pad_left, W, Ho, Wo, Hp, Wp);
        return fail(h, CID_ERR_SHAPE, m);
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
    if (max_forwards < 1 || max_forwards > 4096) return fail(h, CID_ERR_INVALID, "cid_timing_begin: max_forwards out of range");
    if (!h->tev.empty()) return fail(h, CID_ERR_STATE, "cid_timing_begin: timing already armed");
    h->tev.resize((size_t)max_forwards * (NL + 1));
    for (size_t i = 0; i < h->tev.size(); ++i)
        if (hipEventCreate(&h->tev[i]) != hipSuccess) {
            for (size_t j = 0; j < i; ++j) (void)hipEventDestroy(h->tev[j]);
            h->tev.clear();
            return fail(h, CID_ERR_HIP, "cid_timing_begin: hipEventCreate failed");
        }
    h->tev_forwards = max_forwards;
    h->tev_used = 0;
    return CID_OK;
}

int cid_timing_end(cid_handle_t h, void* stream, float* launch_ms_sum, int* forwards) {
    if (!h) return CID_ERR_INVALID;
    if (!launch_ms_sum || !forwards) return fail(h, CID_ERR_INVALID, "cid_timing_end: null pointer");
    if (h->tev.empty()) return fail(h, CID_ERR_STATE, "cid_timing_end: timing not armed");
    int rc = CID_OK;
    if (hipStreamSynchronize(static_cast<hipStream_t>(stream)) != hipSuccess) rc = fail(h, CID_ERR_HIP, "cid_timing_end: stream sync failed");
    for (int l = 0; l < NL; ++l) launch_ms_sum[l] = 0.f;
    for (int f = 0; rc == CID_OK && f < h->tev_used; ++f)
        for (int l = 0; l < NL; ++l) {
            float ms = 0.f;
            const hipEvent_t* e = h->tev.data() + (size_t)f * (NL + 1);
            if (hipEventElapsedTime(&ms, e[l], e[l + 1]) != hipSuccess) { rc = fail(h, CID_ERR_HIP, "cid_timing_end: hipEventElapsedTime failed"); break; }
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
    if (!launch_ms) return fail(h, CID_ERR_INVALID, "cid_forward_timed: null launch_ms");
    hipEvent_t ev[NL + 1];
    int made = 0;
    for (; made <= NL; ++made)
        if (hipEventCreate(&ev[made]) != hipSuccess) break;
    int rc = made == NL + 1 ? CID_OK : fail(h, CID_ERR_HIP, "hipEventCreate failed");
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rc == CID_OK) rc = run_forward(h, in, CID_FMT_F32_NCHW, out, CID_FMT_F32_NCHW, N, H, W, ws, ws_bytes, s, ev);
    if (rc == CID_OK && hipStreamSynchronize(s) != hipSuccess) rc = fail(h, CID_ERR_HIP, "cid_forward_timed: stream sync failed");
    if (rc == CID_OK)
        for (int l = 0; l < NL; ++l)
            if (hipEventElapsedTime(&launch_ms[l], ev[l], ev[l + 1]) != hipSuccess) rc = fail(h, CID_ERR_HIP, "hipEventElapsedTime failed");
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
    if (algo != CID_ALGO_DIRECT && algo != CID_ALGO_WINOGRAD64 && algo != CID_ALGO_WINOGRAD42 && algo != CID_ALGO_SPLIT16) return fail(h, CID_ERR_INVALID, "cid_set_conv_algo: unknown algorithm");
    h->algo = algo;
    return CID_OK;
}
int cid_set_tail_algo(cid_handle_t h, int algo) {
    if (!h) return CID_ERR_INVALID;
    if (algo != CID_TAIL_FUSED && algo != CID_TAIL_BANDS && algo != CID_TAIL_TILES) return fail(h, CID_ERR_INVALID, "cid_set_tail_algo: unknown algorithm");
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
    if (dtype != CID_DTYPE_F32 && dtype != CID_DTYPE_F16) return fail(h, CID_ERR_INVALID, "cid_set_compute_dtype: unknown dtype");
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
    return fail(h, CID_ERR_HIP, std::string(what) + ": " + (rccl().error_string ? rccl().error_string(rc) : "RCCL error"));
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
    if (!comm || root < 0 || rank < 0) return fail(h, CID_ERR_INVALID, "cid_broadcast_weights: null communicator or negative rank");
    if (!h->dev_blob) return fail(h, CID_ERR_STATE, "cid_broadcast_weights: no device blob attached (root: cid_upload_weights; receivers: cid_attach_weights on an allocated buffer)");
    if (!rccl().ok) return fail(h, CID_ERR_STATE, "cid_broadcast_weights: " + rccl().why);
    hipStream_t s = static_cast<hipStream_t>(stream);
    void* blob = const_cast<float*>(h->dev_blob);
    const size_t bytes = kBlob.total * sizeof(float);
    const int rc = rccl().broadcast(blob, blob, bytes, /*ncclUint8*/ 1, root, comm, s);   // in place: one 26 MB message, root -> everyone
    if (rc != 0) return rccl_fail(h, "ncclBroadcast", rc);
    if (rank != root) {   // receivers: refresh the host staging copy, so cid_get_weight / state_dict() return what the kernels use
        hipError_t e = hipMemcpyAsync(h->staging.data(), blob, bytes, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(h, CID_ERR_HIP, std::string("cid_broadcast_weights: ") + hipGetErrorString(e));
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

// ---- image-quality metrics (cid_quality): workspace plan and launch sequence; kernels in quality_kernels.h ----
namespace {

constexpr int kQualityMetrics = CID_METRIC_PSNR | CID_METRIC_SSIM | CID_METRIC_MS_SSIM;
constexpr int kQualityChunk = 65535;   // images per launch (grid y of the tile kernel)

struct QualityPlan {
    int levels;                                  // 1, or 5 with MS-SSIM
    int H[Q_LEVELS], W[Q_LEVELS], tiles_x[Q_LEVELS], tiles[Q_LEVELS], off[Q_LEVELS];
    long long slab_stride;                       // slab rows per image
    size_t pyr_a[Q_LEVELS], pyr_b[Q_LEVELS];     // byte offsets of the pooled planes of levels 1..4
    size_t total;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// Argument checks shared by cid_quality_workspace_bytes and cid_quality (metrics bits, then shape).
int quality_plan(int N, int H, int W, int metrics, QualityPlan& q) {
    if (metrics == 0 || (metrics & ~kQualityMetrics)) return CID_ERR_INVALID;
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((metrics & CID_METRIC_SSIM) && (H < 7 || W < 7)) return CID_ERR_SHAPE;
    if ((metrics & CID_METRIC_MS_SSIM) && (H <= 160 || W <= 160)) return CID_ERR_SHAPE;   // pytorch_msssim: min side > (11-1)*2^4
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;                            // one plane < 2^31 pixels
    q.levels = (metrics & CID_METRIC_MS_SSIM) ? Q_LEVELS : 1;
    long long rows = 0;
    int h = H, w = W;
    for (int l = 0; l < q.levels; ++l) {
        q.H[l] = h;
        q.W[l] = w;
        q.tiles_x[l] = (w + Q_TX - 1) / Q_TX;
        q.tiles[l] = ((h + Q_TY - 1) / Q_TY) * q.tiles_x[l];
        q.off[l] = (int)rows;
        rows += q.tiles[l];
        h = (h + 1) / 2;
        w = (w + 1) / 2;
    }
    q.slab_stride = rows;
    size_t at = align256((size_t)N * rows * QSLOTS * sizeof(double));
    for (int side = 0; side < 2; ++side)
        for (int l = 1; l < q.levels; ++l) {
            (side ? q.pyr_b : q.pyr_a)[l] = at;
            at += align256((size_t)N * 3 * q.H[l] * q.W[l] * sizeof(float));
        }
    q.total = at;
    return CID_OK;
}

// pytorch_msssim _fspecial_gauss_1d(11, 1.5) in float32: exp(-(k-5)^2 / (2*1.5^2)), normalised by its sum.
void gauss_window(float* g) {
    float sum = 0.f;
    for (int k = 0; k < 11; ++k) {
        const float d = (float)(k - 5);
        g[k] = std::exp(-(d * d) / 4.5f);
        sum += g[k];
    }
    for (int k = 0; k < 11; ++k) g[k] /= sum;
}

}  // namespace

extern "C" {

int cid_quality_workspace_bytes(int N, int H, int W, int metrics, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    QualityPlan q;
    const int rc = quality_plan(N, H, W, metrics, q);
    if (rc == CID_OK) *bytes = q.total;
    return rc;
}

int cid_quality(const void* a, int a_fmt, const void* b, int b_fmt, int N, int H, int W, int metrics, double* out,
                void* workspace, size_t workspace_bytes, void* stream) {
    if (!a || !b || !out || !workspace) return CID_ERR_INVALID;
    const auto fmt_ok = [](const void* p, int f) {
        return (f == CID_FMT_U8_NHWC) || (f == CID_FMT_F32_NCHW && ((uintptr_t)p & 3) == 0);
    };
    if (!fmt_ok(a, a_fmt) || !fmt_ok(b, b_fmt) || ((uintptr_t)out & 7)) return CID_ERR_INVALID;
    QualityPlan q;
    const int rc = quality_plan(N, H, W, metrics, q);
    if (rc != CID_OK) return rc;
    if (workspace_bytes < q.total || ((uintptr_t)workspace & 255)) return CID_ERR_WORKSPACE;

    static float g[11];
    static const bool g_ready = (gauss_window(g), true);
    (void)g_ready;
    const hipStream_t s = static_cast<hipStream_t>(stream);
    char* ws = static_cast<char*>(workspace);
    double* part = reinterpret_cast<double*>(ws);
    const bool box = metrics & CID_METRIC_SSIM, gauss = metrics & CID_METRIC_MS_SSIM;

    for (int n0 = 0; n0 < N; n0 += kQualityChunk) {
        const int nc = std::min(kQualityChunk, N - n0);
        for (int l = 0; l < q.levels; ++l) {
            QualityLevelArgs p{};
            p.a = l == 0 ? a : ws + q.pyr_a[l];
            p.b = l == 0 ? b : ws + q.pyr_b[l];
            p.fa = l == 0 ? a_fmt : CID_FMT_F32_NCHW;
            p.fb = l == 0 ? b_fmt : CID_FMT_F32_NCHW;
            p.H = q.H[l];
            p.W = q.W[l];
            p.tiles_x = q.tiles_x[l];
            p.n0 = n0;
            const bool pool = gauss && l + 1 < q.levels;
            p.pa = pool ? reinterpret_cast<float*>(ws + q.pyr_a[l + 1]) : nullptr;
            p.pb = pool ? reinterpret_cast<float*>(ws + q.pyr_b[l + 1]) : nullptr;
            p.part = part + (size_t)q.off[l] * QSLOTS;
            p.slab_stride = q.slab_stride;
            std::memcpy(p.g, g, sizeof g);
            const dim3 grid((unsigned)q.tiles[l], (unsigned)nc), block(Q_THREADS);
            if (l > 0) {
                if (pool) hipLaunchKernelGGL((k_quality_tile<false, false, true, true>), grid, block, 0, s, p);
                else hipLaunchKernelGGL((k_quality_tile<false, false, true, false>), grid, block, 0, s, p);
            } else if (box && gauss) {
                hipLaunchKernelGGL((k_quality_tile<true, true, true, true>), grid, block, 0, s, p);
            } else if (gauss) {
                hipLaunchKernelGGL((k_quality_tile<true, false, true, true>), grid, block, 0, s, p);
            } else if (box) {
                hipLaunchKernelGGL((k_quality_tile<true, true, false, false>), grid, block, 0, s, p);
            } else {
                hipLaunchKernelGGL((k_quality_tile<true, false, false, false>), grid, block, 0, s, p);
            }
            if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
        }
        QualityFinishArgs f{};
        f.part = part;
        f.slab_stride = q.slab_stride;
        f.H = H;
        f.W = W;
        for (int l = 0; l < q.levels; ++l) {
            f.level_tiles[l] = q.tiles[l];
            f.level_off[l] = q.off[l];
        }
        f.levels = q.levels;
        f.metrics = metrics;
        f.n0 = n0;
        f.out = out;
        hipLaunchKernelGGL(k_quality_finish, dim3((unsigned)nc), dim3(64), 0, s, f);
        if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
    }
    return CID_OK;
}

}  // extern "C"

// ---- noise synthesis (cid_add_noise): argument checks and launches; kernels in noise_kernels.h ----
namespace {

// exp(-lambda) for lambda = 0..255 from the host libm (std::exp), the value synth.add_poisson_noise takes from math.exp
const double* poisson_exp_table() {
    static double t[256];
    static const bool ready = [] {
        for (int l = 0; l < 256; ++l) t[l] = std::exp(-(double)l);
        return true;
    }();
    (void)ready;
    return t;
}

static_assert(CID_NOISE_GAUSSIAN == NK_GAUSSIAN && CID_NOISE_SALT_PEPPER == NK_SALT_PEPPER && CID_NOISE_SPECKLE == NK_SPECKLE &&
                  CID_NOISE_POISSON == NK_POISSON && CID_NOISE_UNIFORM == NK_UNIFORM, "noise kind enums out of sync");

}  // namespace

extern "C" {

int cid_add_noise(const void* clean_u8_nhwc, void* out_u8_nhwc, int N, int H, int W, int kind, const double* params, int nparams,
                  uint64_t seed, uint64_t first_index, void* stream) {
    if (!clean_u8_nhwc || !out_u8_nhwc) return CID_ERR_INVALID;
    if (kind < CID_NOISE_GAUSSIAN || kind > CID_NOISE_UNIFORM) return CID_ERR_INVALID;
    const int want = kind == CID_NOISE_POISSON ? 0 : 2;
    if (nparams != want || (want && !params)) return CID_ERR_INVALID;
    for (int i = 0; i < want; ++i)
        if (!std::isfinite(params[i])) return CID_ERR_INVALID;
    if ((kind == CID_NOISE_GAUSSIAN || kind == CID_NOISE_SPECKLE) && params[1] < 0.0) return CID_ERR_INVALID;
    if (kind == CID_NOISE_SALT_PEPPER && (params[0] < 0.0 || params[0] > 1.0 || params[1] < 0.0 || params[1] > 1.0))
        return CID_ERR_INVALID;
    if (kind == CID_NOISE_UNIFORM && params[0] > params[1]) return CID_ERR_INVALID;
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if (kind == CID_NOISE_SALT_PEPPER && (H < 2 || W < 2)) return CID_ERR_SHAPE;
    if ((long long)H * W * 3 >= 0x80000000LL) return CID_ERR_SHAPE;

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const int per = H * W * 3;
    const uint64_t seed0 = seed + first_index;
    const unsigned gy = (unsigned)std::min(N, NOISE_MAX_GRID_Y);

    if (kind == CID_NOISE_SALT_PEPPER) {
        if (out_u8_nhwc != clean_u8_nhwc &&
            hipMemcpyAsync(out_u8_nhwc, clean_u8_nhwc, (size_t)N * per, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return CID_ERR_HIP;
        for (int pass = 0; pass < 2; ++pass) {   // salt, then pepper: stream order makes pepper win a collision
            NoiseScatterArgs a{};
            a.out = static_cast<uint8_t*>(out_u8_nhwc);
            a.N = N;
            a.H = H;
            a.W = W;
            a.draws = (int)((double)per * params[pass]);   // int(float(H*W*3) * prob); <= per
            a.seed0 = seed0;
            a.stream_row = pass ? NS_PEPPER_ROW : NS_SALT_ROW;
            a.stream_col = pass ? NS_PEPPER_COL : NS_SALT_COL;
            a.value = pass ? 0 : 255;
            if (a.draws == 0) continue;
            const dim3 grid((unsigned)((a.draws + NOISE_THREADS - 1) / NOISE_THREADS), gy);
            hipLaunchKernelGGL(k_noise_scatter, grid, dim3(NOISE_THREADS), 0, s, a);
            if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
        }
        return CID_OK;
    }

    NoiseArgs a{};
    a.in = static_cast<const uint8_t*>(clean_u8_nhwc);
    a.out = static_cast<uint8_t*>(out_u8_nhwc);
    a.N = N;
    a.per = per;
    a.seed0 = seed0;
    if (want) {
        a.p0 = params[0];
        a.p1 = params[1];
    }
    const dim3 grid((unsigned)((per + NOISE_THREADS * NOISE_EPT - 1) / (NOISE_THREADS * NOISE_EPT)), gy), block(NOISE_THREADS);
    switch (kind) {
        case CID_NOISE_GAUSSIAN:
            a.stream_a = NS_GAUSS_U1;
            a.stream_b = NS_GAUSS_U2;
            hipLaunchKernelGGL(k_noise_elem<NK_GAUSSIAN>, grid, block, 0, s, a);
            break;
        case CID_NOISE_SPECKLE:
            a.stream_a = NS_SPECKLE_U1;
            a.stream_b = NS_SPECKLE_U2;
            hipLaunchKernelGGL(k_noise_elem<NK_SPECKLE>, grid, block, 0, s, a);
            break;
        case CID_NOISE_UNIFORM:
            a.stream_a = NS_UNIFORM;
            hipLaunchKernelGGL(k_noise_elem<NK_UNIFORM>, grid, block, 0, s, a);
            break;
        default:   // CID_NOISE_POISSON
            a.stream_a = NS_POISSON;
            std::memcpy(a.exp_neg, poisson_exp_table(), sizeof a.exp_neg);
            hipLaunchKernelGGL(k_noise_elem<NK_POISSON>, grid, block, 0, s, a);
            break;
    }
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"

// ---- bicubic resize (cid_resize_*): coefficient tables, tile choice and the launch; kernel in resize_kernels.h ----
namespace {

// Pillow's bicubic filter (a = -0.5), in its evaluation order
double resize_cubic(double t) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (t < 0.0) t = -t;
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1.0;
    if (t < 2.0) return (((t - 5.0) * t + 8.0) * t - 4.0) * a;
    return 0.0;
}

// One axis' tables (include/cid.h states the arithmetic; synth.resize_tables_np restates it): bounds [outS][2] = (min, n), coeffs
// [outS][ksize] 22-bit fixed point, zero past n.
void resize_tables(int inS, int outS, int& ksize, std::vector<int>& bounds, std::vector<int>& coeffs) {
#pragma clang fp contract(off)
    const double scale = (double)inS / (double)outS;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * fs;
    ksize = (int)std::ceil(support) * 2 + 1;
    const double ss = 1.0 / fs;
    bounds.assign((size_t)outS * 2, 0);
    coeffs.assign((size_t)outS * ksize, 0);
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < outS; ++xx) {
        const double center = ((double)xx + 0.5) * scale;
        int xmin = (int)(center - support + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + support + 0.5);
        if (xmax > inS) xmax = inS;
        const int n = xmax - xmin;
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = resize_cubic(((double)(x + xmin) - center + 0.5) * ss);
            ww = ww + w[x];
        }
        int* k = &coeffs[(size_t)xx * ksize];
        for (int x = 0; x < n; ++x) {
            const double v = ww != 0.0 ? w[x] / ww : w[x];
            k[x] = v < 0.0 ? (int)(-0.5 + v * 4194304.0) : (int)(0.5 + v * 4194304.0);
        }
        bounds[2 * (size_t)xx] = xmin;
        bounds[2 * (size_t)xx + 1] = n;
    }
}

constexpr int RESIZE_MAX_SIDE = 16384;
constexpr int RESIZE_MAX_FACTOR = 64;

int pow2_ceil(int v) {
    int p = 1;
    while (p < v) p *= 2;
    return p;
}

// Over the tiles of `tile` outputs of one axis: the widest source span [first.min, last.min + last.n) and each tile's largest n.
int resize_tile_spans(const std::vector<int>& bounds, int outS, int tile, std::vector<int>& tile_n) {
    int widest = 0;
    tile_n.clear();
    for (int t0 = 0; t0 < outS; t0 += tile) {
        const int t1 = std::min(outS, t0 + tile) - 1;
        widest = std::max(widest, bounds[2 * (size_t)t1] + bounds[2 * (size_t)t1 + 1] - bounds[2 * (size_t)t0]);
        int m = 0;
        for (int i = t0; i <= t1; ++i) m = std::max(m, bounds[2 * (size_t)i + 1]);
        tile_n.push_back(m);
    }
    return widest;
}

}  // namespace

struct cid_resize_plan_s {
    int Hs = 0, Ws = 0, Hd = 0, Wd = 0;
    int mode = 0;                          // ResizeMode
    int ksize[2] = {0, 0};                 // axis 0 vertical, 1 horizontal
    std::vector<int> bounds[2], coeffs[2];
    ResizeArgs args{};                     // src, dst, N, f32 are filled in per call
    unsigned tiles = 0;
    size_t lds_bytes = 0;
    int* dev = nullptr;                    // the device copy of the tables; null on a machine without a GPU
    int device = -1;
};

extern "C" {

int cid_resize_plan_create(cid_resize_plan_t* out, int Hs, int Ws, int Hd, int Wd, int filter) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (filter != CID_RESAMPLE_BICUBIC) return CID_ERR_INVALID;
    if (Hs < 1 || Ws < 1 || Hd < 1 || Wd < 1) return CID_ERR_SHAPE;
    if (Hs > RESIZE_MAX_SIDE || Ws > RESIZE_MAX_SIDE || Hd > RESIZE_MAX_SIDE || Wd > RESIZE_MAX_SIDE) return CID_ERR_SHAPE;
    if ((long long)Hs * Ws * 3 >= 0x80000000LL || (long long)Hd * Wd * 3 >= 0x80000000LL) return CID_ERR_SHAPE;
    if ((long long)Hs > (long long)RESIZE_MAX_FACTOR * Hd || (long long)Ws > (long long)RESIZE_MAX_FACTOR * Wd) return CID_ERR_SHAPE;

    auto* p = new cid_resize_plan_s;
    p->Hs = Hs; p->Ws = Ws; p->Hd = Hd; p->Wd = Wd;
    resize_tables(Hs, Hd, p->ksize[0], p->bounds[0], p->coeffs[0]);
    resize_tables(Ws, Wd, p->ksize[1], p->bounds[1], p->coeffs[1]);
    // what the kernel relies on: spans that move monotonically (a tile's span is first.min .. last.min + last.n) and
    // coefficients that fit the 24-bit multiply
    for (int ax = 0; ax < 2; ++ax) {
        const int outS = ax ? Wd : Hd;
        const std::vector<int>& b = p->bounds[ax];
        bool ok = true;
        for (int i = 0; i < outS; ++i) {
            if (b[2 * (size_t)i + 1] < 1) ok = false;
            if (i && (b[2 * (size_t)i] < b[2 * (size_t)i - 2] || b[2 * (size_t)i] + b[2 * (size_t)i + 1] < b[2 * (size_t)i - 2] + b[2 * (size_t)i - 1])) ok = false;
        }
        for (int k : p->coeffs[ax])
            if (k <= -(1 << 23) || k >= (1 << 23)) ok = false;
        if (!ok) {
            delete p;
            return CID_ERR_SHAPE;
        }
    }
    const bool hpass = Ws != Wd, vpass = Hs != Hd;
    p->mode = hpass ? (vpass ? RM_BOTH : RM_HONLY) : (vpass ? RM_VONLY : RM_COPY);

    // tile: about 4 pixels per lane, 64 columns wide where the image is; halved until band + stage fit the LDS budget
    int TC = std::min(64, pow2_ceil(Wd)), TR = std::min(pow2_ceil(Hd), 1024 / TC);
    std::vector<int> vtn, htn;
    int band_pitch = 0, band_bytes = 0, stage_pitch = 0, nband = 0;
    for (;;) {
        nband = vpass ? resize_tile_spans(p->bounds[0], Hd, TR, vtn) : TR;
        const int nsrc = hpass ? resize_tile_spans(p->bounds[1], Wd, TC, htn) : TC;
        if (!vpass) vtn.assign((size_t)cdiv(Hd, TR), 0);
        if (!hpass) htn.assign((size_t)cdiv(Wd, TC), 0);
        band_pitch = p->mode == RM_BOTH ? TC * 3 : p->mode == RM_VONLY ? (15 + TC * 3 + 15) / 16 * 16 : 0;
        band_bytes = (band_pitch * nband + 15) / 16 * 16;
        stage_pitch = hpass ? (15 + nsrc * 3 + 15) / 16 * 16 : 0;
        if (band_bytes + stage_pitch <= RESIZE_LDS_BUDGET) break;
        if (TR > 1 && (band_bytes > RESIZE_LDS_BUDGET / 2 || TC == 1)) TR /= 2;
        else if (TC > 1) TC /= 2;
        else {   // a 1 x 1 tile needs at most 258 band rows of 32 bytes and one stage row of 3 * 258 + 30 bytes
            delete p;
            return CID_ERR_SHAPE;
        }
    }
    ResizeArgs& a = p->args;
    a.Hs = Hs; a.Ws = Ws; a.Hd = Hd; a.Wd = Wd;
    a.TR = TR; a.TC = TC;
    a.tiles_x = cdiv(Wd, TC);
    a.band_pitch = band_pitch;
    a.band_bytes = band_bytes;
    a.stage_pitch = stage_pitch;
    a.SR = hpass ? std::max(1, std::min(nband, (RESIZE_LDS_BUDGET - band_bytes) / stage_pitch)) : 0;
    a.h.ksize = p->ksize[1];
    a.v.ksize = p->ksize[0];
    p->tiles = (unsigned)a.tiles_x * (unsigned)cdiv(Hd, TR);
    p->lds_bytes = (size_t)band_bytes + (size_t)a.SR * stage_pitch;

    // the device copy: vertical bounds, coefficients, tile maxima; horizontal bounds, TRANSPOSED coefficients, tile maxima.
    // Without a GPU the plan keeps its host tables only (cid_resize_plan_table works; cid_resize returns CID_ERR_STATE).
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) {
        (void)hipGetLastError();
        *out = p;
        return CID_OK;
    }
    std::vector<int> blob;
    const auto put = [&blob](const std::vector<int>& v) {
        const size_t at = blob.size();
        blob.insert(blob.end(), v.begin(), v.end());
        return at;
    };
    const size_t o_vb = put(p->bounds[0]), o_vc = put(p->coeffs[0]), o_vt = put(vtn), o_hb = put(p->bounds[1]);
    std::vector<int> hT((size_t)p->ksize[1] * Wd);
    for (int x = 0; x < Wd; ++x)
        for (int k = 0; k < p->ksize[1]; ++k) hT[(size_t)k * Wd + x] = p->coeffs[1][(size_t)x * p->ksize[1] + k];
    const size_t o_hc = put(hT), o_ht = put(htn);
    if (hipGetDevice(&p->device) != hipSuccess || hipMalloc(reinterpret_cast<void**>(&p->dev), blob.size() * sizeof(int)) != hipSuccess ||
        hipMemcpy(p->dev, blob.data(), blob.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) {
        if (p->dev) (void)hipFree(p->dev);
        delete p;
        return CID_ERR_HIP;
    }
    a.v.bounds = p->dev + o_vb; a.v.coeffs = p->dev + o_vc; a.v.tile_n = p->dev + o_vt;
    a.h.bounds = p->dev + o_hb; a.h.coeffs = p->dev + o_hc; a.h.tile_n = p->dev + o_ht;
    *out = p;
    return CID_OK;
}

void cid_resize_plan_destroy(cid_resize_plan_t p) {
    if (!p) return;
    if (p->dev) (void)hipFree(p->dev);
    delete p;
}

int cid_resize_plan_table(cid_resize_plan_t p, int axis, int* ksize, int* bounds, int* coeffs) {
    if (!p || !ksize || (axis != 0 && axis != 1)) return CID_ERR_INVALID;
    *ksize = p->ksize[axis];
    if (bounds) std::memcpy(bounds, p->bounds[axis].data(), p->bounds[axis].size() * sizeof(int));
    if (coeffs) std::memcpy(coeffs, p->coeffs[axis].data(), p->coeffs[axis].size() * sizeof(int));
    return CID_OK;
}

int cid_resize(cid_resize_plan_t p, const void* src_u8_nhwc, void* dst, int dst_fmt, int N, void* stream) {
    if (!p || !src_u8_nhwc || !dst) return CID_ERR_INVALID;
    if (dst_fmt != CID_FMT_U8_NHWC && dst_fmt != CID_FMT_F32_NCHW) return CID_ERR_INVALID;
    if (dst_fmt == CID_FMT_F32_NCHW && ((uintptr_t)dst & 3)) return CID_ERR_INVALID;
    if (N < 1) return CID_ERR_INVALID;
    if (!p->dev) return CID_ERR_STATE;   // created without a GPU
    ResizeArgs a = p->args;
    a.src = static_cast<const uint8_t*>(src_u8_nhwc);
    a.dst = dst;
    a.N = N;
    a.f32 = dst_fmt == CID_FMT_F32_NCHW;
    const dim3 grid(p->tiles, (unsigned)std::min(N, RESIZE_MAX_GRID_Y)), block(RESIZE_THREADS);
    const hipStream_t s = static_cast<hipStream_t>(stream);
    switch (p->mode) {
        case RM_BOTH: hipLaunchKernelGGL(k_resize<RM_BOTH>, grid, block, p->lds_bytes, s, a); break;
        case RM_HONLY: hipLaunchKernelGGL(k_resize<RM_HONLY>, grid, block, p->lds_bytes, s, a); break;
        case RM_VONLY: hipLaunchKernelGGL(k_resize<RM_VONLY>, grid, block, p->lds_bytes, s, a); break;
        default: hipLaunchKernelGGL(k_resize<RM_COPY>, grid, block, 0, s, a); break;
    }
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

}  // extern "C"

// ---- the trainer's discriminator (cid_disc_*): weight packing, workspace plan and launch sequence; kernels in disc_kernels.h ----
namespace {

struct DiscConvDef { const char* name; int cin, cout, k, stride; };
constexpr int kDiscConvs = 5;
constexpr DiscConvDef kDiscConv[kDiscConvs] = {
    {"model.0", 3, 64, 3, 1}, {"model.2", 64, 64, 3, 2}, {"model.5", 64, 128, 3, 1}, {"model.8", 128, 128, 3, 2}, {"model.12", 128, 1, 1, 1},
};
constexpr int kDiscBnC[3] = {64, 128, 128};
constexpr int kDiscChunk = 65535;   // images per launch (grid y of the conv kernels, grid x of the head)

// Blob segments (floats, each 64-float aligned): weights then biases of each convolution.  Layer 0 and 12 keep the reference
// layout; layers 2, 5, 8 are packed [CIN/8][9 taps][8][COUT] (DiscConvArgs::w) with the biases right behind.
struct DiscBlob {
    size_t off[kDiscConvs], total;
    DiscBlob() : off{}, total(0) {
        size_t at = 0;
        for (int i = 0; i < kDiscConvs; ++i) {
            off[i] = at;
            const auto& L = kDiscConv[i];
            at += (size_t)L.cout * L.cin * L.k * L.k + L.cout;
            at = (at + 63) & ~(size_t)63;
        }
        total = at;
    }
};
const DiscBlob kDiscBlob;

struct DiscPlan {
    int H2, W2, H4, W4;
    int tiles_x[3], tiles[3];           // conv launches 2, 5, 8
    size_t regA, regB, st, slab[3], total;
};

constexpr int kDiscTileRows[3] = {DiscGeom<64, 64, 2>::TH, DiscGeom<64, 128, 1>::TH, DiscGeom<128, 128, 2>::TH};

int disc_plan(int N, int H, int W, int training, DiscPlan& p) {
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;   // the layer-0 kernel indexes an image's pixels with int
    p.H2 = (H - 1) / 2 + 1;
    p.W2 = (W - 1) / 2 + 1;
    p.H4 = (p.H2 - 1) / 2 + 1;
    p.W4 = (p.W2 - 1) / 2 + 1;
    if (training && (long long)N * p.H4 * p.W4 == 1) return CID_ERR_SHAPE;
    const int ho[3] = {p.H2, p.H2, p.H4}, wo[3] = {p.W2, p.W2, p.W4};
    for (int l = 0; l < 3; ++l) {
        p.tiles_x[l] = (wo[l] + D_TW - 1) / D_TW;
        p.tiles[l] = ((ho[l] + kDiscTileRows[l] - 1) / kDiscTileRows[l]) * p.tiles_x[l];
    }
    const size_t n = (size_t)N, f = sizeof(float);
    // region A: a0 (64 x H x W), later z5 (128 x H2 x W2); region B: z2 (64 x H2 x W2), later z8 (128 x H4 x W4)
    const size_t a = std::max(n * 64 * H * W, n * 128 * p.H2 * p.W2) * f;
    const size_t b = std::max(n * 64 * p.H2 * p.W2, n * 128 * p.H4 * p.W4) * f;
    size_t at = 0;
    p.regA = at;
    at += align256(a);
    p.regB = at;
    at += align256(b);
    p.st = at;
    at += align256(3 * 128 * 2 * f);
    const int couts[3] = {64, 128, 128};
    for (int l = 0; l < 3; ++l) {
        p.slab[l] = at;
        if (training) at += align256((size_t)couts[l] * 2 * n * p.tiles[l] * sizeof(double));
    }
    p.total = at;
    return CID_OK;
}

template <int CIN, int COUT, int S, bool BN_IN>
hipError_t disc_conv_launch(const DiscConvArgs& base, int layer, const DiscPlan& p, int N, bool training, hipStream_t s) {
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        DiscConvArgs a = base;
        a.n0 = n0;
        a.tiles_x = p.tiles_x[layer];
        a.tiles = p.tiles[layer];
        const dim3 grid((unsigned)p.tiles[layer], (unsigned)std::min(kDiscChunk, N - n0)), block(D_THREADS);
        if (training) hipLaunchKernelGGL((k_disc_conv<CIN, COUT, S, BN_IN, true>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((k_disc_conv<CIN, COUT, S, BN_IN, false>), grid, block, 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

bool disc_finite_nonneg(double v) { return std::isfinite(v) && v >= 0.0; }

}  // namespace

struct cid_disc_s {
    std::vector<float> staging = std::vector<float>(kDiscBlob.total, 0.f);
    bool have[kDiscConvs][2] = {};
    const float* dev_blob = nullptr;
    std::string err;
};

namespace {
int dfail(cid_disc_t d, int code, const std::string& msg) {
    if (d) d->err = msg;
    return code;
}

// Where one forward keeps its tensors: two overlapping workspace regions (cid_disc_forward) or a per-call buffer (cid_disc_forward_saved).
struct DiscBufs {
    float *a0, *z2, *z5, *z8;
    float* st[3];      // (scale, shift) pairs of the three BatchNorms
    double* mi[3];     // (mean, invstd) pairs, or null
    double* slab[3];   // train mode: per-tile partial sums
};

// The argument checks every forward entry point shares, in the order cid.h documents; `buf` is its workspace or saved buffer.
int disc_check_forward(cid_disc_t d, const char* fn, const void* in, int in_fmt, const float* out, int N, int H, int W,
                       const cid_disc_bn* bn, int training, const void* buf, DiscPlan& p) {
    const std::string f = std::string(fn) + ": ";
    if (!in || !out || !bn || !buf) return dfail(d, CID_ERR_INVALID, f + "null pointer");
    if (in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) return dfail(d, CID_ERR_INVALID, f + "unknown input format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || ((uintptr_t)out & 3))
        return dfail(d, CID_ERR_INVALID, f + "misaligned fp32 operand");
    if (training != 0 && training != 1) return dfail(d, CID_ERR_INVALID, f + "training must be 0 or 1");
    for (int l = 0; l < 3; ++l) {
        const cid_disc_bn& b = bn[l];
        if (!b.gamma || !b.beta || !b.running_mean || !b.running_var || (training && !b.num_batches_tracked))
            return dfail(d, CID_ERR_INVALID, f + "null BatchNorm pointer");
        if (!disc_finite_nonneg(b.eps)) return dfail(d, CID_ERR_INVALID, f + "eps must be finite and >= 0");
        if (training && !(disc_finite_nonneg(b.momentum) || b.momentum == CID_DISC_MOMENTUM_NONE))
            return dfail(d, CID_ERR_INVALID, f + "momentum must be finite and >= 0, or CID_DISC_MOMENTUM_NONE");
    }
    if (disc_plan(N, H, W, training, p) != CID_OK)
        return dfail(d, CID_ERR_SHAPE, training && N >= 1 && H >= 1 && W >= 1 && (long long)H * W <= 0x7fffffffLL
                                           ? "Expected more than 1 value per channel when training"
                                           : f + "input shape not accepted (N, H, W >= 1, H*W < 2^31)");
    return CID_OK;
}

// The forward's launch sequence on checked arguments.
int disc_forward_run(cid_disc_t d, const char* fn, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn,
                     int training, const DiscPlan& p, const DiscBufs& b, hipStream_t s) {
    const float* blob = d->dev_blob;
    const auto herr = [&](const char* what) { return dfail(d, CID_ERR_HIP, std::string(fn) + ": " + what + ": " + hipGetErrorString(hipGetLastError())); };

    if (!training) {
        DiscBnEvalArgs e{};
        for (int l = 0; l < 3; ++l) {
            e.gamma[l] = bn[l].gamma;
            e.beta[l] = bn[l].beta;
            e.running_mean[l] = bn[l].running_mean;
            e.running_var[l] = bn[l].running_var;
            e.eps[l] = bn[l].eps;
            e.st[l] = b.st[l];
            e.C[l] = kDiscBnC[l];
            e.mi[l] = b.mi[l];
        }
        hipLaunchKernelGGL(k_disc_bn_eval, dim3(3), dim3(128), 0, s, e);
        if (hipPeekAtLastError() != hipSuccess) return herr("bn_eval");
    }
    // layer 0
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        DiscConv0Args a{in, b.a0, blob + kDiscBlob.off[0], H, W, n0};
        const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), (unsigned)std::min(kDiscChunk, N - n0));
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_disc_conv0<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_disc_conv0<false>, grid, dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("conv0");
    }
    const auto stats = [&](int l, long long pix) {
        DiscStatsArgs a{};
        a.slab = b.slab[l];
        a.rows = (long long)N * p.tiles[l];
        a.count = (double)N * (double)pix;
        a.gamma = bn[l].gamma;
        a.beta = bn[l].beta;
        a.running_mean = bn[l].running_mean;
        a.running_var = bn[l].running_var;
        a.num_batches_tracked = reinterpret_cast<const long long*>(bn[l].num_batches_tracked);
        a.eps = bn[l].eps;
        a.momentum = bn[l].momentum == CID_DISC_MOMENTUM_NONE ? -1.0 : bn[l].momentum;
        a.st = b.st[l];
        a.mi = b.mi[l];
        hipLaunchKernelGGL(k_disc_bn_stats, dim3(kDiscBnC[l]), dim3(D_THREADS), 0, s, a);
        return hipPeekAtLastError();
    };
    const auto conv_args = [&](const float* src, float* dst, int ci, const float* st_in, int l, int Hin, int Win, int Ho, int Wo) {
        DiscConvArgs a{};
        a.in = src;
        a.out = dst;
        a.w = blob + kDiscBlob.off[ci];
        a.st_in = st_in;
        a.slab = training ? b.slab[l] : nullptr;
        a.rows = (long long)N * p.tiles[l];
        a.Hin = Hin;
        a.Win = Win;
        a.Ho = Ho;
        a.Wo = Wo;
        return a;
    };
    // layer 2 (reads a0, writes z2), BN3
    if (disc_conv_launch<64, 64, 2, false>(conv_args(b.a0, b.z2, 1, nullptr, 0, H, W, p.H2, p.W2), 0, p, N, training, s) != hipSuccess)
        return herr("conv2");
    if (training && stats(0, (long long)p.H2 * p.W2) != hipSuccess) return herr("bn3 stats");
    // layer 5 (reads z2 through BN3 + LeakyReLU, writes z5), BN6
    if (disc_conv_launch<64, 128, 1, true>(conv_args(b.z2, b.z5, 2, b.st[0], 1, p.H2, p.W2, p.H2, p.W2), 1, p, N, training, s) != hipSuccess)
        return herr("conv5");
    if (training && stats(1, (long long)p.H2 * p.W2) != hipSuccess) return herr("bn6 stats");
    // layer 8 (reads z5 through BN6 + LeakyReLU, writes z8), BN9
    if (disc_conv_launch<128, 128, 2, true>(conv_args(b.z5, b.z8, 3, b.st[1], 2, p.H2, p.W2, p.H4, p.W4), 2, p, N, training, s) != hipSuccess)
        return herr("conv8");
    if (training && stats(2, (long long)p.H4 * p.W4) != hipSuccess) return herr("bn9 stats");
    // head: BN9 + LeakyReLU, average pool, 1x1 conv, sigmoid
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        DiscHeadArgs a{b.z8, b.st[2], blob + kDiscBlob.off[4], out, (long long)p.H4 * p.W4, n0};
        hipLaunchKernelGGL(k_disc_head, dim3((unsigned)std::min(kDiscChunk, N - n0)), dim3(D_HEAD_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("head");
    }
    if (training) {
        hipLaunchKernelGGL(k_disc_bn_count, dim3(1), dim3(64), 0, s, reinterpret_cast<long long*>(bn[0].num_batches_tracked),
                           reinterpret_cast<long long*>(bn[1].num_batches_tracked), reinterpret_cast<long long*>(bn[2].num_batches_tracked));
        if (hipPeekAtLastError() != hipSuccess) return herr("bn count");
    }
    return CID_OK;
}
}  // namespace

extern "C" {

int cid_disc_create(cid_disc_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = new (std::nothrow) cid_disc_s();
    return *out ? CID_OK : CID_ERR_INVALID;
}

void cid_disc_destroy(cid_disc_t d) { delete d; }

const char* cid_disc_last_error(cid_disc_t d) { return d ? d->err.c_str() : "null handle"; }

int cid_disc_set_weight(cid_disc_t d, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!d) return CID_ERR_INVALID;
    if (!key || !data || (!shape && ndim > 0)) return dfail(d, CID_ERR_INVALID, "cid_disc_set_weight: null argument");
    const std::string k(key);
    int li = -1, is_bias = 0;
    for (int i = 0; i < kDiscConvs; ++i) {
        if (k == std::string(kDiscConv[i].name) + ".weight") { li = i; is_bias = 0; }
        if (k == std::string(kDiscConv[i].name) + ".bias") { li = i; is_bias = 1; }
    }
    if (li < 0)
        return dfail(d, CID_ERR_KEY, "cid_disc_set_weight: unknown key '" + k +
                                         "' (BatchNorm tensors model.3/6/9 are passed to cid_disc_forward, not staged)");
    const auto& L = kDiscConv[li];
    const int64_t want_w[4] = {L.cout, L.cin, L.k, L.k};
    const bool ok = is_bias ? (ndim == 1 && shape[0] == L.cout)
                            : (ndim == 4 && std::equal(shape, shape + 4, want_w));
    if (!ok) return dfail(d, CID_ERR_SHAPE, "cid_disc_set_weight: size mismatch for " + k);
    float* seg = d->staging.data() + kDiscBlob.off[li];
    const size_t nw = (size_t)L.cout * L.cin * L.k * L.k;
    const bool packed = li >= 1 && li <= 3;
    if (is_bias) {
        std::memcpy(seg + nw, data, (size_t)L.cout * sizeof(float));
    } else if (!packed) {
        std::memcpy(seg, data, nw * sizeof(float));
    } else {
        for (int co = 0; co < L.cout; ++co)
            for (int ci = 0; ci < L.cin; ++ci)
                for (int tap = 0; tap < 9; ++tap)
                    seg[((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * L.cout + co] = data[((size_t)co * L.cin + ci) * 9 + tap];
    }
    d->have[li][is_bias] = true;
    return CID_OK;
}

size_t cid_disc_packed_weights_bytes(void) { return kDiscBlob.total * sizeof(float); }

int cid_disc_upload_weights(cid_disc_t d, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    if (!device_blob) return dfail(d, CID_ERR_INVALID, "cid_disc_upload_weights: null device pointer");
    if ((uintptr_t)device_blob & 255) return dfail(d, CID_ERR_WORKSPACE, "cid_disc_upload_weights: blob must be 256-byte aligned");
    for (int i = 0; i < kDiscConvs; ++i)
        if (!d->have[i][0] || !d->have[i][1])
            return dfail(d, CID_ERR_STATE, std::string("cid_disc_upload_weights: ") + kDiscConv[i].name + " not set");
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(device_blob, d->staging.data(), kDiscBlob.total * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // staging is pageable host memory owned by the handle
    if (e != hipSuccess) return dfail(d, CID_ERR_HIP, std::string("cid_disc_upload_weights: ") + hipGetErrorString(e));
    d->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_disc_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    const int rc = disc_plan(N, H, W, training, p);
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

int cid_disc_forward(cid_disc_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn,
                     int training, void* workspace, size_t workspace_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    DiscPlan p;
    const int rc = disc_check_forward(d, "cid_disc_forward", in, in_fmt, out, N, H, W, bn, training, workspace, p);
    if (rc != CID_OK) return rc;
    if (workspace_bytes < p.total || ((uintptr_t)workspace & 255))
        return dfail(d, CID_ERR_WORKSPACE, "cid_disc_forward: workspace smaller than cid_disc_workspace_bytes() or not 256-byte aligned");
    if (!d->dev_blob) return dfail(d, CID_ERR_STATE, "cid_disc_forward: weights not uploaded");
    char* ws = static_cast<char*>(workspace);
    DiscBufs b{};
    b.a0 = b.z5 = reinterpret_cast<float*>(ws + p.regA);
    b.z2 = b.z8 = reinterpret_cast<float*>(ws + p.regB);
    for (int l = 0; l < 3; ++l) {
        b.st[l] = reinterpret_cast<float*>(ws + p.st) + l * 256;
        b.slab[l] = reinterpret_cast<double*>(ws + p.slab[l]);
    }
    return disc_forward_run(d, "cid_disc_forward", in, in_fmt, out, N, H, W, bn, training, p, b, static_cast<hipStream_t>(stream));
}

// ---- backward pass: the per-call saved buffer, the workspace plan and the launch sequence; kernels in disc_bwd_kernels.h ----
}  // extern "C"

namespace {

// What cid_disc_forward_saved keeps for one call.
struct DiscSavedPlan {
    size_t a0, z2, z5, z8, st, mi, slab[3], total;
};

void disc_saved_plan(int N, int H, int W, int training, const DiscPlan& p, DiscSavedPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t o = at;
        at += align256(bytes);
        return o;
    };
    q.a0 = take(n * 64 * H * W * f);
    q.z2 = take(n * 64 * p.H2 * p.W2 * f);
    q.z5 = take(n * 128 * p.H2 * p.W2 * f);
    q.z8 = take(n * 128 * p.H4 * p.W4 * f);
    q.st = take(3 * 256 * f);
    q.mi = take(3 * 256 * sizeof(double));
    const int couts[3] = {64, 128, 128};
    for (int l = 0; l < 3; ++l) q.slab[l] = training ? take((size_t)couts[l] * 2 * n * p.tiles[l] * sizeof(double)) : at;
    q.total = at;
}

DiscBufs disc_saved_bufs(void* saved, const DiscSavedPlan& q) {
    char* sv = static_cast<char*>(saved);
    DiscBufs b{};
    b.a0 = reinterpret_cast<float*>(sv + q.a0);
    b.z2 = reinterpret_cast<float*>(sv + q.z2);
    b.z5 = reinterpret_cast<float*>(sv + q.z5);
    b.z8 = reinterpret_cast<float*>(sv + q.z8);
    for (int l = 0; l < 3; ++l) {
        b.st[l] = reinterpret_cast<float*>(sv + q.st) + l * 256;
        b.mi[l] = reinterpret_cast<double*>(sv + q.mi) + l * 256;
        b.slab[l] = reinterpret_cast<double*>(sv + q.slab[l]);
    }
    return b;
}

// Workspace of one backward call.  X holds the gradient of a6 and later of a0, Y the gradient of a3 (the forward's two regions).
struct DiscBwdPlan {
    int strips[3];                  // BatchNorm strips per image
    int wg_tiles_x[3], wg_tiles[3]; // wgrad items per image of layers 2, 5, 8
    int wg_splits[3];
    int dg_tiles_x[3], dg_tiles[3]; // dgrad tiles of the largest class
    int w0_strips, w0_splits;
    size_t dl, mean, coef, bnslab, X, Y, part, part_b, part0, total;
};

constexpr int kDiscWgCD[3] = {64, 128, 128}, kDiscWgCX[3] = {64, 64, 128}, kDiscWgS[3] = {2, 1, 2};
constexpr int kDiscDgTileRows[3] = {DiscDgradGeom<64, 64, 2>::TH, DiscDgradGeom<128, 64, 1>::TH, DiscDgradGeom<128, 128, 2>::TH};

void disc_bwd_plan(int N, int H, int W, const DiscPlan& p, DiscBwdPlan& q) {
    const size_t n = (size_t)N, f = sizeof(float);
    const int ho[3] = {p.H2, p.H2, p.H4}, wo[3] = {p.W2, p.W2, p.W4};
    const int hin[3] = {H, p.H2, p.H2}, win[3] = {W, p.W2, p.W2};
    size_t bnslab = 0, part = 0, part_b = 0;
    for (int l = 0; l < 3; ++l) {
        q.strips[l] = (int)(((long long)ho[l] * wo[l] + D_BN_STRIP - 1) / D_BN_STRIP);
        bnslab = std::max(bnslab, (size_t)kDiscBnC[l] * 2 * n * q.strips[l] * sizeof(double));
        q.wg_tiles_x[l] = (wo[l] + D_TW - 1) / D_TW;
        q.wg_tiles[l] = ((ho[l] + D_WG_TH - 1) / D_WG_TH) * q.wg_tiles_x[l];
        const long long items = (long long)N * q.wg_tiles[l];
        q.wg_splits[l] = (int)std::min<long long>(items, 512 / (kDiscWgCX[l] / 16));
        part = std::max(part, (size_t)q.wg_splits[l] * kDiscWgCX[l] * kDiscWgCD[l] * 9 * f);
        part_b = std::max(part_b, (size_t)q.wg_splits[l] * kDiscWgCD[l] * sizeof(double));
        const int hc = (hin[l] + kDiscWgS[l] - 1) / kDiscWgS[l], wc = (win[l] + kDiscWgS[l] - 1) / kDiscWgS[l];
        q.dg_tiles_x[l] = (wc + D_TW - 1) / D_TW;
        q.dg_tiles[l] = ((hc + kDiscDgTileRows[l] - 1) / kDiscDgTileRows[l]) * q.dg_tiles_x[l];
    }
    q.w0_strips = (int)(((long long)H * W + 63) / 64);
    q.w0_splits = (int)std::min<long long>((long long)N * q.w0_strips, 1024);
    size_t at = 0;
    const auto take = [&](size_t bytes) {
        const size_t o = at;
        at += align256(bytes);
        return o;
    };
    q.dl = take(n * f);
    q.mean = take(n * 128 * sizeof(double));
    q.coef = take(3 * 128 * D_COEF * f);
    q.bnslab = take(bnslab);
    q.X = take(std::max(n * 128 * p.H2 * p.W2, n * 64 * H * W) * f);
    q.Y = take(n * 64 * p.H2 * p.W2 * f);
    q.part = take(part);
    q.part_b = take(part_b);
    q.part0 = take((size_t)q.w0_splits * 64 * 28 * sizeof(double));
    q.total = at;
}

template <int CD, int CX, int S, bool BN_IN, bool HEAD>
hipError_t disc_wgrad_launch(const DiscWgradArgs& a, float* dw, float* db, hipStream_t s) {
    hipLaunchKernelGGL((k_disc_wgrad<CD, CX, S, BN_IN, HEAD>), dim3((unsigned)a.splits, CX / 16), dim3(D_THREADS), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const DiscWgradReduceArgs r{a.part, a.part_b, dw, db, a.splits, CD, CX};
    hipLaunchKernelGGL(k_disc_wgrad_reduce, dim3((CD * CX * 9 + CD + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, s, r);
    return hipGetLastError();
}

template <int CD, int CX, int S, bool HEAD>
hipError_t disc_dgrad_launch(const DiscDgradArgs& base, int tiles, int N, hipStream_t s) {
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        DiscDgradArgs a = base;
        a.n0 = n0;
        const dim3 grid((unsigned)tiles, (unsigned)std::min(kDiscChunk, N - n0), DiscDgradGeom<CD, CX, S>::CLASSES);
        hipLaunchKernelGGL((k_disc_dgrad<CD, CX, S, HEAD>), grid, dim3(D_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

template <int C, bool HEAD>
hipError_t disc_bn_part_launch(const DiscBnPartArgs& base, int N, hipStream_t s) {
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        DiscBnPartArgs a = base;
        a.n0 = n0;
        hipLaunchKernelGGL((k_disc_bn_bwd_part<C, HEAD>), dim3((unsigned)a.strips, (unsigned)std::min(kDiscChunk, N - n0)), dim3(D_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// Shape checks shared by the backward entry points.
int disc_bwd_shape(cid_disc_t d, const char* fn, int N, int H, int W, int training, DiscPlan& p) {
    if (training != 0 && training != 1) return dfail(d, CID_ERR_INVALID, std::string(fn) + ": training must be 0 or 1");
    if (disc_plan(N, H, W, training, p) != CID_OK)
        return dfail(d, CID_ERR_SHAPE, std::string(fn) + ": shape not accepted (N, H, W >= 1, H*W < 2^31, more than one value per channel in train mode)");
    return CID_OK;
}

}  // namespace

extern "C" {

int cid_disc_saved_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    const int rc = disc_plan(N, H, W, training, p);
    if (rc != CID_OK) return rc;
    DiscSavedPlan q;
    disc_saved_plan(N, H, W, training, p, q);
    *bytes = q.total;
    return CID_OK;
}

int cid_disc_forward_saved(cid_disc_t d, const void* in, int in_fmt, float* out, int N, int H, int W, const cid_disc_bn* bn,
                           int training, void* saved, size_t saved_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    DiscPlan p;
    const int rc = disc_check_forward(d, "cid_disc_forward_saved", in, in_fmt, out, N, H, W, bn, training, saved, p);
    if (rc != CID_OK) return rc;
    DiscSavedPlan q;
    disc_saved_plan(N, H, W, training, p, q);
    if (saved_bytes < q.total || ((uintptr_t)saved & 255))
        return dfail(d, CID_ERR_WORKSPACE, "cid_disc_forward_saved: saved buffer smaller than cid_disc_saved_bytes() or not 256-byte aligned");
    if (!d->dev_blob) return dfail(d, CID_ERR_STATE, "cid_disc_forward_saved: weights not uploaded");
    return disc_forward_run(d, "cid_disc_forward_saved", in, in_fmt, out, N, H, W, bn, training, p, disc_saved_bufs(saved, q),
                            static_cast<hipStream_t>(stream));
}

int cid_disc_backward_workspace_bytes(int N, int H, int W, int training, size_t* bytes) {
    if (!bytes || (training != 0 && training != 1)) return CID_ERR_INVALID;
    DiscPlan p;
    const int rc = disc_plan(N, H, W, training, p);
    if (rc != CID_OK) return rc;
    DiscBwdPlan q;
    disc_bwd_plan(N, H, W, p, q);
    *bytes = q.total;
    return CID_OK;
}

int cid_disc_backward(cid_disc_t d, const void* in, int in_fmt, const float* grad_prob, int N, int H, int W, const cid_disc_bn* bn,
                      int training, const void* saved, size_t saved_bytes, const cid_disc_grads* g, void* workspace,
                      size_t workspace_bytes, void* stream) {
    if (!d) return CID_ERR_INVALID;
    const char* fn = "cid_disc_backward";
    if (!in || !grad_prob || !bn || !saved || !g || !workspace) return dfail(d, CID_ERR_INVALID, "cid_disc_backward: null pointer");
    if (in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) return dfail(d, CID_ERR_INVALID, "cid_disc_backward: unknown input format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || ((uintptr_t)grad_prob & 3))
        return dfail(d, CID_ERR_INVALID, "cid_disc_backward: misaligned fp32 operand");
    for (int l = 0; l < 3; ++l)
        if (!bn[l].gamma) return dfail(d, CID_ERR_INVALID, "cid_disc_backward: null BatchNorm weight pointer");
    bool misaligned = ((uintptr_t)g->input & 3) != 0;
    for (int i = 0; i < 5; ++i) misaligned = misaligned || ((uintptr_t)g->w[i] & 3) || ((uintptr_t)g->b[i] & 3);
    for (int l = 0; l < 3; ++l) misaligned = misaligned || ((uintptr_t)g->gamma[l] & 3) || ((uintptr_t)g->beta[l] & 3);
    if (misaligned) return dfail(d, CID_ERR_INVALID, "cid_disc_backward: misaligned gradient pointer");
    if (g->input && in_fmt != CID_FMT_F32_NCHW)
        return dfail(d, CID_ERR_INVALID, "cid_disc_backward: a uint8 input has no gradient (grads.input must be null)");
    DiscPlan p;
    const int rc = disc_bwd_shape(d, fn, N, H, W, training, p);
    if (rc != CID_OK) return rc;
    DiscSavedPlan sp;
    disc_saved_plan(N, H, W, training, p, sp);
    if (saved_bytes < sp.total || ((uintptr_t)saved & 255))
        return dfail(d, CID_ERR_WORKSPACE, "cid_disc_backward: saved buffer smaller than cid_disc_saved_bytes() or not 256-byte aligned");
    DiscBwdPlan q;
    disc_bwd_plan(N, H, W, p, q);
    if (workspace_bytes < q.total || ((uintptr_t)workspace & 255))
        return dfail(d, CID_ERR_WORKSPACE, "cid_disc_backward: workspace smaller than cid_disc_backward_workspace_bytes() or not 256-byte aligned");
    if (!d->dev_blob) return dfail(d, CID_ERR_STATE, "cid_disc_backward: weights not uploaded");

    const hipStream_t s = static_cast<hipStream_t>(stream);
    const DiscBufs sv = disc_saved_bufs(const_cast<void*>(saved), sp);
    char* ws = static_cast<char*>(workspace);
    float* dl = reinterpret_cast<float*>(ws + q.dl);
    double* mean = reinterpret_cast<double*>(ws + q.mean);
    float* coef[3];
    for (int l = 0; l < 3; ++l) coef[l] = reinterpret_cast<float*>(ws + q.coef) + l * 128 * D_COEF;
    double* bnslab = reinterpret_cast<double*>(ws + q.bnslab);
    float* X = reinterpret_cast<float*>(ws + q.X);
    float* Y = reinterpret_cast<float*>(ws + q.Y);
    float* part = reinterpret_cast<float*>(ws + q.part);
    double* part_b = reinterpret_cast<double*>(ws + q.part_b);
    double* part0 = reinterpret_cast<double*>(ws + q.part0);
    const float* blob = d->dev_blob;
    const auto herr = [&](const char* what) { return dfail(d, CID_ERR_HIP, std::string(fn) + ": " + what + ": " + hipGetErrorString(hipGetLastError())); };

    // what is asked for at or below each stage: head(8) > bn9(7) > conv8(6) > bn6(5) > conv5(4) > bn3(3) > conv2(2) > conv0(1) > input(0)
    const bool want[9] = {g->input != nullptr, g->w[0] || g->b[0], g->w[1] || g->b[1], g->gamma[0] || g->beta[0], g->w[2] || g->b[2],
                          g->gamma[1] || g->beta[1], g->w[3] || g->b[3], g->gamma[2] || g->beta[2], g->w[4] || g->b[4]};
    bool below[10];   // below[k]: something at a stage < k is asked for
    below[0] = false;
    for (int k = 0; k < 9; ++k) below[k + 1] = below[k] || want[k];
    if (!below[9]) return CID_OK;
    const long long P4 = (long long)p.H4 * p.W4, P2 = (long long)p.H2 * p.W2;

    // head
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        DiscHeadBwdArgs a{sv.z8, sv.st[2], blob + kDiscBlob.off[4], grad_prob, mean, dl, P4, n0};
        hipLaunchKernelGGL(k_disc_head_bwd, dim3((unsigned)std::min(kDiscChunk, N - n0)), dim3(D_HEAD_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("head");
    }
    {
        DiscHeadReduceArgs a{mean, dl, blob + kDiscBlob.off[4], g->w[4], g->b[4], coef[2], (double)P4, N};
        hipLaunchKernelGGL(k_disc_head_reduce, dim3(1), dim3(128), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("head reduce");
    }
    if (!below[8]) return CID_OK;

    const auto bn_reduce = [&](int l, long long pix) {
        DiscBnRedArgs a{bnslab, (long long)N * q.strips[l], (double)N * (double)pix, bn[l].gamma, sv.st[l], sv.mi[l], training,
                        coef[l], g->gamma[l], g->beta[l]};
        hipLaunchKernelGGL(k_disc_bn_bwd_reduce, dim3(kDiscBnC[l]), dim3(D_THREADS), 0, s, a);
        return hipPeekAtLastError();
    };
    const auto bn_part = [&](int l, const float* z, const float* up, long long pix) {
        DiscBnPartArgs a{z, up, dl, coef[l], sv.st[l], sv.mi[l], bnslab, (long long)N * q.strips[l], pix, q.strips[l], 0};
        return a;
    };
    const auto wg_args = [&](int l, const DiscDzSrc& dz, const float* ain, const float* st_in, int Hin, int Win, int Ho, int Wo) {
        DiscWgradArgs a{};
        a.dz = dz;
        a.ain = ain;
        a.st_in = st_in;
        a.part = part;
        a.part_b = part_b;
        a.items = (long long)N * q.wg_tiles[l];
        a.splits = q.wg_splits[l];
        a.Hin = Hin;
        a.Win = Win;
        a.Ho = Ho;
        a.Wo = Wo;
        a.tiles_x = q.wg_tiles_x[l];
        a.tiles = q.wg_tiles[l];
        return a;
    };
    const auto dg_args = [&](int l, int ci, const DiscDzSrc& dz, float* out, int Hin, int Win, int Ho, int Wo) {
        DiscDgradArgs a{};
        a.dz = dz;
        a.w = blob + kDiscBlob.off[ci];
        a.out = out;
        a.Hin = Hin;
        a.Win = Win;
        a.Ho = Ho;
        a.Wo = Wo;
        a.tiles_x = q.dg_tiles_x[l];
        return a;
    };

    // BN9 (upstream: the head's dl[n] * w12[c] / P4), layer 8
    if (disc_bn_part_launch<128, true>(bn_part(2, sv.z8, nullptr, P4), N, s) != hipSuccess) return herr("bn9 sums");
    if (bn_reduce(2, P4) != hipSuccess) return herr("bn9 reduce");
    const DiscDzSrc dz8{sv.z8, nullptr, dl, coef[2]};
    if (want[6] && disc_wgrad_launch<128, 128, 2, true, true>(wg_args(2, dz8, sv.z5, sv.st[1], p.H2, p.W2, p.H4, p.W4), g->w[3], g->b[3], s) != hipSuccess)
        return herr("wgrad8");
    if (!below[6]) return CID_OK;
    if (disc_dgrad_launch<128, 128, 2, true>(dg_args(2, 3, dz8, X, p.H2, p.W2, p.H4, p.W4), q.dg_tiles[2], N, s) != hipSuccess) return herr("dgrad8");
    // BN6, layer 5
    if (disc_bn_part_launch<128, false>(bn_part(1, sv.z5, X, P2), N, s) != hipSuccess) return herr("bn6 sums");
    if (bn_reduce(1, P2) != hipSuccess) return herr("bn6 reduce");
    const DiscDzSrc dz5{sv.z5, X, nullptr, coef[1]};
    if (want[4] && disc_wgrad_launch<128, 64, 1, true, false>(wg_args(1, dz5, sv.z2, sv.st[0], p.H2, p.W2, p.H2, p.W2), g->w[2], g->b[2], s) != hipSuccess)
        return herr("wgrad5");
    if (!below[4]) return CID_OK;
    if (disc_dgrad_launch<128, 64, 1, false>(dg_args(1, 2, dz5, Y, p.H2, p.W2, p.H2, p.W2), q.dg_tiles[1], N, s) != hipSuccess) return herr("dgrad5");
    // BN3, layer 2
    if (disc_bn_part_launch<64, false>(bn_part(0, sv.z2, Y, P2), N, s) != hipSuccess) return herr("bn3 sums");
    if (bn_reduce(0, P2) != hipSuccess) return herr("bn3 reduce");
    const DiscDzSrc dz2{sv.z2, Y, nullptr, coef[0]};
    if (want[2] && disc_wgrad_launch<64, 64, 2, false, false>(wg_args(0, dz2, sv.a0, nullptr, H, W, p.H2, p.W2), g->w[1], g->b[1], s) != hipSuccess)
        return herr("wgrad2");
    if (!below[2]) return CID_OK;
    if (disc_dgrad_launch<64, 64, 2, false>(dg_args(0, 1, dz2, X, H, W, p.H2, p.W2), q.dg_tiles[0], N, s) != hipSuccess) return herr("dgrad2");
    // layer 0
    if (want[1]) {
        DiscWgrad0Args a{in, sv.a0, X, part0, (long long)N * q.w0_strips, q.w0_splits, q.w0_strips, H, W};
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_disc_wgrad0<true>, dim3((unsigned)q.w0_splits), dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_disc_wgrad0<false>, dim3((unsigned)q.w0_splits), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("wgrad0");
        DiscWgrad0ReduceArgs r{part0, g->w[0], g->b[0], q.w0_splits};
        hipLaunchKernelGGL(k_disc_wgrad0_reduce, dim3((64 * 28 + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, s, r);
        if (hipPeekAtLastError() != hipSuccess) return herr("wgrad0 reduce");
    }
    if (want[0]) {
        for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
            DiscDgrad0Args a{sv.a0, X, blob + kDiscBlob.off[0], g->input, H, W, n0};
            const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), (unsigned)std::min(kDiscChunk, N - n0));
            hipLaunchKernelGGL(k_disc_dgrad0, grid, dim3(D_THREADS), 0, s, a);
            if (hipPeekAtLastError() != hipSuccess) return herr("dgrad0");
        }
    }
    return CID_OK;
}

int cid_disc_pack_weights_device(cid_disc_t d, const float* const* dev_params, void* device_blob, void* stream) {
    if (!d) return CID_ERR_INVALID;
    if (!dev_params || !device_blob) return dfail(d, CID_ERR_INVALID, "cid_disc_pack_weights_device: null pointer");
    for (int i = 0; i < CID_DISC_NUM_WEIGHTS; ++i)
        if (!dev_params[i] || ((uintptr_t)dev_params[i] & 3))
            return dfail(d, CID_ERR_INVALID, "cid_disc_pack_weights_device: null or misaligned parameter pointer");
    if ((uintptr_t)device_blob & 255) return dfail(d, CID_ERR_WORKSPACE, "cid_disc_pack_weights_device: blob must be 256-byte aligned");
    DiscPackArgs a{};
    for (int i = 0; i < kDiscConvs; ++i) {
        a.w[i] = dev_params[2 * i];
        a.b[i] = dev_params[2 * i + 1];
        a.off[i] = (int)kDiscBlob.off[i];
        a.cin[i] = kDiscConv[i].cin;
        a.cout[i] = kDiscConv[i].cout;
        a.kk[i] = kDiscConv[i].k * kDiscConv[i].k;
    }
    a.blob = static_cast<float*>(device_blob);
    a.total = (int)kDiscBlob.total;
    hipLaunchKernelGGL(k_disc_pack, dim3((a.total + D_THREADS - 1) / D_THREADS), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
    if (hipGetLastError() != hipSuccess) return dfail(d, CID_ERR_HIP, "cid_disc_pack_weights_device: launch failed");
    d->dev_blob = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_disc_saved_masks(const void* saved, size_t saved_bytes, int N, int H, int W, int training, unsigned char* const* masks, void* stream) {
    if (!saved || !masks || (training != 0 && training != 1)) return CID_ERR_INVALID;
    for (int i = 0; i < 4; ++i)
        if (!masks[i]) return CID_ERR_INVALID;
    DiscPlan p;
    const int rc = disc_plan(N, H, W, training, p);
    if (rc != CID_OK) return rc;
    DiscSavedPlan sp;
    disc_saved_plan(N, H, W, training, p, sp);
    if (saved_bytes < sp.total || ((uintptr_t)saved & 255)) return CID_ERR_WORKSPACE;
    const DiscBufs sv = disc_saved_bufs(const_cast<void*>(saved), sp);
    const float* z[4] = {sv.a0, sv.z2, sv.z5, sv.z8};
    const float* st[4] = {nullptr, sv.st[0], sv.st[1], sv.st[2]};
    const int C[4] = {64, 64, 128, 128};
    const long long P[4] = {(long long)H * W, (long long)p.H2 * p.W2, (long long)p.H2 * p.W2, (long long)p.H4 * p.W4};
    for (int i = 0; i < 4; ++i) {
        DiscMaskArgs a{z[i], st[i], masks[i], (long long)N * C[i] * P[i], P[i], C[i]};
        const long long blocks = (a.total + D_THREADS - 1) / D_THREADS;
        if (blocks > 0x7fffffffLL) return CID_ERR_SHAPE;
        hipLaunchKernelGGL(k_disc_masks, dim3((unsigned)blocks), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
        if (hipGetLastError() != hipSuccess) return CID_ERR_HIP;
    }
    return CID_OK;
}

int cid_disc_losses(const float* p_real, const float* p_fake, const void* den, int d_fmt, const void* clean, int c_fmt,
                    int N, int H, int W, double* out, void* stream) {
    if (!p_real || !p_fake || !den || !clean || !out) return CID_ERR_INVALID;
    const auto fmt_ok = [](const void* q, int f) {
        return (f == CID_FMT_U8_NHWC) || (f == CID_FMT_F32_NCHW && ((uintptr_t)q & 3) == 0);
    };
    if (!fmt_ok(den, d_fmt) || !fmt_ok(clean, c_fmt) || ((uintptr_t)p_real & 3) || ((uintptr_t)p_fake & 3) || ((uintptr_t)out & 7))
        return CID_ERR_INVALID;
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    DiscLossArgs a{p_real, p_fake, den, clean, d_fmt, c_fmt, N, (long long)H * W, out};
    hipLaunchKernelGGL(k_disc_losses, dim3(1), dim3(D_LOSS_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

// ---- the optimizer step (optim_kernels.h) ----
}  // extern "C"
namespace {
// cid_adam_step's argument checks and k_adam_step's arguments; a.nent == 0: nothing to launch.
int adam_plan(const cid_adam_tensor* tensors, int ntensors, const cid_adam_hyper* hp, AdamArgs& a) {
    static_assert(CID_ADAM_MAX_TENSORS == ADAM_MAX_TENSORS, "cid.h and optim_kernels.h disagree");
    if (!tensors || !hp) return CID_ERR_INVALID;
    if (ntensors < 1 || ntensors > CID_ADAM_MAX_TENSORS) return CID_ERR_INVALID;
    for (int i = 0; i < ntensors; ++i) {
        const cid_adam_tensor& t = tensors[i];
        if (t.count <= 0) continue;
        const void* q[4] = {t.param, t.grad, t.exp_avg, t.exp_avg_sq};
        for (const void* x : q)
            if (!x || ((uintptr_t)x & 3)) return CID_ERR_INVALID;
    }
    for (int i = 0; i < ntensors; ++i)
        if (tensors[i].count < 0 || tensors[i].step < 1) return CID_ERR_INVALID;
    const auto in_range = [](double x, double hi_excl) { return std::isfinite(x) && x >= 0.0 && x < hi_excl; };
    const double inf = std::numeric_limits<double>::infinity();
    if (!in_range(hp->lr, inf) || !in_range(hp->beta1, 1.0) || !in_range(hp->beta2, 1.0) || !in_range(hp->eps, inf) ||
        !in_range(hp->weight_decay, inf))
        return CID_ERR_INVALID;

    // No written range may meet another written range or a gradient: sweep over the ranges in address order with the furthest end of
    // the written and of the read ranges seen so far.
    struct Range { uintptr_t lo, hi; bool written; };
    Range r[4 * CID_ADAM_MAX_TENSORS];
    int nr = 0;
    a.nent = 0;
    unsigned long long items = 0;
    for (int i = 0; i < ntensors; ++i) {
        const cid_adam_tensor& t = tensors[i];
        if (t.count == 0) continue;
        if (t.count > (int64_t)1 << 44) return CID_ERR_INVALID;   // beyond any device memory; keeps the byte ranges and the grid in range
        const uintptr_t bytes = (uintptr_t)t.count * 4;
        r[nr++] = {(uintptr_t)t.param, (uintptr_t)t.param + bytes, true};
        r[nr++] = {(uintptr_t)t.exp_avg, (uintptr_t)t.exp_avg + bytes, true};
        r[nr++] = {(uintptr_t)t.exp_avg_sq, (uintptr_t)t.exp_avg_sq + bytes, true};
        r[nr++] = {(uintptr_t)t.grad, (uintptr_t)t.grad + bytes, false};
        AdamEntry& e = a.ent[a.nent++];
        e.param = t.param;
        e.grad = t.grad;
        e.exp_avg = t.exp_avg;
        e.exp_avg_sq = t.exp_avg_sq;
        e.count = t.count;
        e.t0 = (unsigned)items;
        const unsigned mis = (unsigned)((uintptr_t)t.param & 15);
        const bool same = ((uintptr_t)t.grad & 15) == mis && ((uintptr_t)t.exp_avg & 15) == mis && ((uintptr_t)t.exp_avg_sq & 15) == mis;
        e.off = same ? mis / 4 : ADAM_SCALAR;   // mis / 4 phantom elements in front put quad q at byte 16 q - mis of the tensor: 16-byte aligned
        items += ((unsigned long long)t.count + (same ? mis / 4 : 0) + ADAM_ITEM_ELEMS - 1) / ADAM_ITEM_ELEMS;
        if (items > 0x7fffffffULL) return CID_ERR_INVALID;
        const double t_d = (double)t.step;
        e.step_size = hp->lr / (1.0 - std::pow(hp->beta1, t_d));
        e.bc2_sqrt = std::sqrt(1.0 - std::pow(hp->beta2, t_d));
    }
    std::sort(r, r + nr, [](const Range& x, const Range& y) { return x.lo < y.lo; });
    uintptr_t wend = 0, rend = 0;
    for (int i = 0; i < nr; ++i) {
        if (r[i].lo < wend || (r[i].written && r[i].lo < rend)) return CID_ERR_INVALID;
        uintptr_t& end = r[i].written ? wend : rend;
        end = std::max(end, r[i].hi);
    }
    a.beta1 = hp->beta1;
    a.one_minus_beta1 = 1.0 - hp->beta1;
    a.beta2 = hp->beta2;
    a.one_minus_beta2 = 1.0 - hp->beta2;
    a.eps = hp->eps;
    a.weight_decay = hp->weight_decay;
    a.nitems = (unsigned)items;
    return CID_OK;
}
}  // namespace
extern "C" {

int cid_adam_step(const cid_adam_tensor* tensors, int ntensors, const cid_adam_hyper* hp, void* stream) {
    AdamArgs a;
    const int rc = adam_plan(tensors, ntensors, hp, a);
    if (rc != CID_OK || a.nent == 0) return rc;
    hipLaunchKernelGGL(k_adam_step, dim3(a.nitems), dim3(ADAM_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipGetLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

int cid_debug_adam_step_host(const cid_adam_tensor* tensors, int ntensors, const cid_adam_hyper* hp) {
    AdamArgs a;
    const int rc = adam_plan(tensors, ntensors, hp, a);
    if (rc != CID_OK || a.nent == 0) return rc;
    for (unsigned item = 0; item < a.nitems; ++item)
        for (unsigned tid = 0; tid < (unsigned)ADAM_THREADS; ++tid) adam_item(a, item, tid);
    return CID_OK;
}

}  // extern "C"

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
    const auto take = [&](size_t bytes) {
        const size_t o = at;
        at += align256(bytes);
        return o;
    };
    q.dz16 = take(s0 * 3 * f);
    q.G4 = take(s0 * 64 * f);
    q.dcat1 = take(s0 * 128 * f);
    q.gd2 = take(s1 * 128 * f);
    q.gt3 = take(s1 * 128 * f);
    q.dcat2 = take(s1 * 256 * f);
    q.gbt = take(s2 * 256 * f);
    q.gt2 = take(s2 * 256 * f);
    q.dp2 = take(s2 * 128 * f);
    q.dp1 = take(s1 * 64 * f);
    q.part = take(part);
    q.part_b = take(part_b);
    q.part27 = take((size_t)q.w27_splits * 64 * 28 * sizeof(double));
    q.part27_b = take((size_t)q.w27_splits * 3 * sizeof(double));
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
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        a.n0 = n0;
        const dim3 grid((unsigned)(a.tiles * (a.CX / CXB)), (unsigned)std::min(kDiscChunk, N - n0));
        hipLaunchKernelGGL((k_gen_dgrad<CD, CXB, TAPS>), grid, dim3(G_THREADS), 0, s, a);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
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
    if (!in || !out || !saved) return fail(h, CID_ERR_INVALID, "cid_forward_saved: null pointer");
    if (h->dtype != CID_DTYPE_F32) return fail(h, CID_ERR_STATE, "cid_forward_saved: the differentiable forward needs compute dtype CID_DTYPE_F32");
    Dims d;
    if (const char* why = gen_bwd_shape_error(N, H, W, d)) {
        char m[384];
        std::snprintf(m, sizeof m, "cid_forward_saved: input [%d,3,%d,%d] not accepted: %s", N, H, W, why);
        return fail(h, CID_ERR_SHAPE, m);
    }
    if (saved_bytes < make_plan(d).total_bytes || ((uintptr_t)saved & 255))
        return fail(h, CID_ERR_WORKSPACE, "cid_forward_saved: saved buffer smaller than cid_saved_bytes() or not 256-byte aligned");
    if (!h->dev_blob) return fail(h, CID_ERR_STATE, "cid_forward_saved: no device weights attached (call cid_upload_weights or cid_attach_weights)");
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
    const char* fn = "cid_backward";
    if (!in || !out || !grad_out || !saved || !g || !workspace) return fail(h, CID_ERR_INVALID, "cid_backward: null pointer");
    if (h->dtype != CID_DTYPE_F32) return fail(h, CID_ERR_STATE, "cid_backward: the backward pass needs compute dtype CID_DTYPE_F32");
    bool misaligned = ((uintptr_t)in & 3) || ((uintptr_t)out & 3) || ((uintptr_t)grad_out & 3) || ((uintptr_t)g->input & 3);
    for (int l = 0; l < NL; ++l) misaligned = misaligned || ((uintptr_t)g->w[l] & 3) || ((uintptr_t)g->b[l] & 3);
    if (misaligned) return fail(h, CID_ERR_INVALID, "cid_backward: misaligned fp32 pointer");
    Dims d;
    if (const char* why = gen_bwd_shape_error(N, H, W, d)) {
        char m[384];
        std::snprintf(m, sizeof m, "cid_backward: input [%d,3,%d,%d] not accepted: %s", N, H, W, why);
        return fail(h, CID_ERR_SHAPE, m);
    }
    const Plan p = make_plan(d);
    if (saved_bytes < p.total_bytes || ((uintptr_t)saved & 255))
        return fail(h, CID_ERR_WORKSPACE, "cid_backward: saved buffer smaller than cid_saved_bytes() or not 256-byte aligned");
    GenBwdPlan q;
    gen_bwd_plan(d, q);
    if (workspace_bytes < q.total || ((uintptr_t)workspace & 255))
        return fail(h, CID_ERR_WORKSPACE, "cid_backward: workspace smaller than cid_backward_workspace_bytes() or not 256-byte aligned");
    if (!h->dev_blob) return fail(h, CID_ERR_STATE, "cid_backward: no device weights attached (call cid_upload_weights or cid_attach_weights)");

    const hipStream_t s = static_cast<hipStream_t>(stream);
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
    const auto herr = [&](const char* what) { return fail(h, CID_ERR_HIP, std::string(fn) + ": " + what + ": " + hipGetErrorString(hipGetLastError())); };

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
        if (hipPeekAtLastError() != hipSuccess) return herr("dz16");
    }
    if (need[11]) {
        const GenWgrad27Args a{dz16, B[T4], 64, 0, part27, part27_b, (long long)N * q.w27_strips, q.w27_splits, q.w27_strips, H, W};
        hipLaunchKernelGGL(k_gen_wgrad27<true>, dim3((unsigned)q.w27_splits), dim3(G_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("upconv1.2 weight gradient");
        const GenWgrad27ReduceArgs r{part27, part27_b, g->w[11], g->b[11], q.w27_splits};
        hipLaunchKernelGGL(k_gen_wgrad27_reduce<true>, dim3((unsigned)cdiv(64 * 28 + 3, G_THREADS)), dim3(G_THREADS), 0, s, r);
        if (hipPeekAtLastError() != hipSuccess) return herr("upconv1.2 weight gradient reduce");
    }
    if (!below[11]) return CID_OK;
    {
        const long long pixels = (long long)N * H * W;
        const GenDgradTailArgs a{dz16, blob + kBlob.raw_w_off[11], B[T4], G4, pixels, H, W};
        hipLaunchKernelGGL(k_gen_dgrad_tail, dim3((unsigned)((pixels + 63) / 64)), dim3(G_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("upconv1.2 data gradient");
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
            if (gen_wgrad(wg, a, g->w[l], g->b[l], s) != hipSuccess) return herr((std::string(kLayers[l].name) + " weight gradient").c_str());
        }
        if (!below[l]) return CID_OK;
        GenDgradArgs a{};
        a.dz = r.dz.p; a.dz_ps = r.dz.ps; a.dz_coff = r.dz.coff;
        a.w = blob + kBlob.raw_w_off[l];
        a.act = r.act; a.act_ps = r.act_ps; a.act_coff = 0;
        a.out = r.dout; a.out_ps = r.out_ps; a.out_coff = 0;
        a.H = r.Ho; a.W = r.Wo; a.CX = kLayers[l].cin;
        if (gen_dgrad(l, a, N, s) != hipSuccess) return herr((std::string(kLayers[l].name) + " data gradient").c_str());
        if (l == 4 || l == 2) {   // the pooled tensor's gradient is complete: finish dz of the skip tensor under it
            GenPoolBwdArgs pa{};
            const int C = l == 4 ? 128 : 64;
            pa.e = l == 4 ? B[CAT2] : B[CAT1]; pa.e_ps = 2 * C; pa.e_coff = C;
            pa.dp = l == 4 ? dp2 : dp1;
            pa.io = l == 4 ? dcat2 : dcat1; pa.io_ps = 2 * C; pa.io_coff = C;
            pa.Hp = r.Ho; pa.Wp = r.Wo;
            pa.total = (long long)N * r.Ho * r.Wo * (C / 4);
            const long long blocks = (pa.total + G_THREADS - 1) / G_THREADS;
            if (blocks > 0x7fffffffLL) return fail(h, CID_ERR_SHAPE, "cid_backward: batch too large for one call");
            if (l == 4) hipLaunchKernelGGL(k_gen_pool_bwd<128>, dim3((unsigned)blocks), dim3(G_THREADS), 0, s, pa);
            else hipLaunchKernelGGL(k_gen_pool_bwd<64>, dim3((unsigned)blocks), dim3(G_THREADS), 0, s, pa);
            if (hipPeekAtLastError() != hipSuccess) return herr("max-pool gradient");
        }
    }

    // down1.0
    if (need[0]) {
        const GenWgrad27Args a{in, gt0, 64, 0, part27, part27_b, (long long)N * q.w27_strips, q.w27_splits, q.w27_strips, H, W};
        hipLaunchKernelGGL(k_gen_wgrad27<false>, dim3((unsigned)q.w27_splits), dim3(G_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("down1.0 weight gradient");
        const GenWgrad27ReduceArgs r{part27, part27_b, g->w[0], g->b[0], q.w27_splits};
        hipLaunchKernelGGL(k_gen_wgrad27_reduce<false>, dim3((unsigned)cdiv(64 * 28, G_THREADS)), dim3(G_THREADS), 0, s, r);
        if (hipPeekAtLastError() != hipSuccess) return herr("down1.0 weight gradient reduce");
    }
    if (g->input) {
        for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
            const GenDgradHeadArgs a{gt0, blob + kBlob.raw_w_off[0], g->input, H, W, n0};
            const dim3 grid((unsigned)(((long long)H * W + G_THREADS - 1) / G_THREADS), (unsigned)std::min(kDiscChunk, N - n0));
            hipLaunchKernelGGL(k_gen_dgrad_head, grid, dim3(G_THREADS), 0, s, a);
            if (hipPeekAtLastError() != hipSuccess) return herr("down1.0 data gradient");
        }
    }
    return CID_OK;
}

}  // extern "C"

// ---- the server's ESRGANGenerator (cid_esr_*): weight staging, BatchNorm folding, workspace plan and launch sequence; kernels in
// esrgan_kernels.h ----
namespace {

constexpr int kEsrMaxBlocks = CID_ESR_MAX_RESIDUALS;
constexpr size_t kEsrHeadSeg = (size_t)E_HEAD_K * 64 + 128;      // weights, bias[64], slope (padded to 64)
constexpr size_t kEsrConvSeg = (size_t)E_CONV_W + 256;           // weights, bias[64], s[64], t[64], slope (padded to 64)
constexpr size_t kEsrTailSeg = (size_t)E_TAIL_W + 64;            // weights, bias[3] (padded to 64)

// The key tables and pack steps below stand on WeightStore (weight_store.h).  What SRGAN shares with ESRGAN is written once here.
void keys_head9(KeyTable& k) {
    k.conv("initial.0.", 64, 3, 9);
    k.tensor("initial.1.weight", {1});
}

// <blk>0 conv, <blk>1 BatchNorm, <blk>2 PReLU, <blk>3 conv, <blk>4 BatchNorm
void keys_res_block(KeyTable& k, const std::string& blk) {
    for (int c = 0; c < 2; ++c) {
        k.conv(blk + std::to_string(3 * c) + ".", 64, 64, 3);
        k.batchnorm(blk + std::to_string(3 * c + 1) + ".", 64);
        if (c == 0) k.tensor(blk + "2.weight", {1});
    }
}

KeyTable esr_keys(int R) {
    KeyTable k;
    keys_head9(k);
    for (int i = 0; i < R; ++i) keys_res_block(k, "residuals." + std::to_string(i) + ".block.");
    k.conv("final.", 3, 64, 9);
    return k;
}

// The BatchNorm under the key prefix `bn` folded to y = s*z + t with s = gamma / sqrt(running_var + eps), t = beta - running_mean * s,
// derived in fp64 and rounded once to fp32.
void pack_bn_fold(const WeightStore& w, const std::string& bn, double eps, int C, float* s_out, float* t_out) {
    const float *gamma = w.get(bn + "weight"), *beta = w.get(bn + "bias"), *mean = w.get(bn + "running_mean"), *var = w.get(bn + "running_var");
    for (int ch = 0; ch < C; ++ch) {
        const double s = (double)gamma[ch] / std::sqrt((double)var[ch] + eps);
        s_out[ch] = (float)s;
        t_out[ch] = (float)((double)beta[ch] - (double)mean[ch] * s);
    }
}

// A 64-channel convolution's [co][K] weights as the [k][64] rows a head kernel reads.
void pack_k64(float* dst, const float* w, int K) {
    for (int co = 0; co < 64; ++co)
        for (int k = 0; k < K; ++k) dst[(size_t)k * 64 + co] = w[(size_t)co * K + k];
}

// initial.*, the 9x9 head: [ci][kh][kw][co], bias, the PReLU's slope
void pack_head9(const WeightStore& w, float* seg) {
    pack_k64(seg, w.get("initial.0.weight"), E_HEAD_K);
    std::memcpy(seg + E_HEAD_K * 64, w.get("initial.0.bias"), 64 * sizeof(float));
    seg[E_HEAD_K * 64 + 64] = w.get("initial.1.weight")[0];
}

// One 3x3 64 -> 64 convolution into k_esr_conv's segment layout.
void pack_conv64(float* seg, const float* w, const float* bias) {
    for (int co = 0; co < 64; ++co)
        for (int ci = 0; ci < 64; ++ci)
            for (int tap = 0; tap < 9; ++tap) seg[((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * 64 + co] = w[((size_t)co * 64 + ci) * 9 + tap];
    std::memcpy(seg + E_CONV_BIAS, bias, 64 * sizeof(float));
}

// Convolution c (0, 1) of the residual block under `blk` with its BatchNorm folded; the first one carries the block's PReLU slope.
void pack_res_conv(const WeightStore& w, float* seg, const std::string& blk, int c, double eps) {
    const std::string conv = blk + std::to_string(3 * c) + ".", bn = blk + std::to_string(3 * c + 1) + ".";
    pack_conv64(seg, w.get(conv + "weight"), w.get(conv + "bias"));
    pack_bn_fold(w, bn, eps, 64, seg + E_CONV_S, seg + E_CONV_T);
    seg[E_CONV_SLOPE] = c == 0 ? w.get(blk + "2.weight")[0] : 0.f;
}

// final.*, the 9x9 tail: [ci][kh][co * 9 + kw], bias
void pack_tail9(const WeightStore& w, float* seg) {
    const float* f = w.get("final.weight");
    for (int co = 0; co < 3; ++co)
        for (int ci = 0; ci < 64; ++ci)
            for (int kh = 0; kh < 9; ++kh)
                for (int kw = 0; kw < 9; ++kw)
                    seg[((size_t)ci * 9 + kh) * E_TAIL_WROW + co * 9 + kw] = f[(((size_t)co * 64 + ci) * 9 + kh) * 9 + kw];
    std::memcpy(seg + E_TAIL_W, w.get("final.bias"), 3 * sizeof(float));
}

// The argument checks cid_esr_forward and cid_sr_forward share.
int check_image_io(WeightStore* h, const std::string& fn, const void* in, int in_fmt, const void* out, int out_fmt, const void* workspace) {
    if (!in || !out || !workspace) return h->fail(CID_ERR_INVALID, fn + ": null pointer");
    if ((in_fmt != CID_FMT_F32_NCHW && in_fmt != CID_FMT_U8_NHWC) || (out_fmt != CID_FMT_F32_NCHW && out_fmt != CID_FMT_U8_NHWC))
        return h->fail(CID_ERR_INVALID, fn + ": unknown format");
    if ((in_fmt == CID_FMT_F32_NCHW && ((uintptr_t)in & 3)) || (out_fmt == CID_FMT_F32_NCHW && ((uintptr_t)out & 3)))
        return h->fail(CID_ERR_INVALID, fn + ": misaligned fp32 operand");
    return CID_OK;
}

struct EsrPlan {
    size_t x1, mid, cur, total;   // byte offsets of the three C8 tensors; `cur` ends as the tensor the tail reads
    int ctiles_x, ctiles, ttiles_x, ttiles;
};

int esr_plan(int N, int H, int W, EsrPlan& p) {
    if (N < 1 || H < 1 || W < 1) return CID_ERR_SHAPE;
    if ((long long)H * W > 0x7fffffffLL) return CID_ERR_SHAPE;   // a pixel index inside one image is an int
    const size_t t = align256((size_t)N * 64 * H * W * sizeof(float));
    p.x1 = 0;
    p.mid = t;
    p.cur = 2 * t;
    p.total = 3 * t;
    p.ctiles_x = (W + D_TW - 1) / D_TW;
    p.ctiles = ((H + DiscGeom<64, 64, 1>::TH - 1) / DiscGeom<64, 64, 1>::TH) * p.ctiles_x;
    p.ttiles_x = (W + E_TAIL_TW - 1) / E_TAIL_TW;
    p.ttiles = ((H + E_TAIL_TH - 1) / E_TAIL_TH) * p.ttiles_x;
    return CID_OK;
}

}  // namespace

struct cid_esr_s : WeightStore {
    int R = 0;
    double eps[2 * kEsrMaxBlocks];
    size_t blob_floats() const { return kEsrHeadSeg + 2 * (size_t)R * kEsrConvSeg + kEsrTailSeg; }
};

namespace {
// The blob from the staged tensors: the head, the 2 R block convolutions, the tail.
void esr_pack(const cid_esr_s* h, float* b) {
    pack_head9(*h, b);
    for (int l = 0; l < 2 * h->R; ++l)
        pack_res_conv(*h, b + kEsrHeadSeg + (size_t)l * kEsrConvSeg, "residuals." + std::to_string(l / 2) + ".block.", l % 2, h->eps[l]);
    pack_tail9(*h, b + kEsrHeadSeg + 2 * (size_t)h->R * kEsrConvSeg);
}
}  // namespace

extern "C" {

int cid_esr_create(cid_esr_t* out, int num_residuals) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (num_residuals < 0 || num_residuals > kEsrMaxBlocks) return CID_ERR_INVALID;
    cid_esr_s* h = new (std::nothrow) cid_esr_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_esr", esr_keys(num_residuals));
    h->R = num_residuals;
    std::fill(h->eps, h->eps + 2 * kEsrMaxBlocks, 1e-5);
    *out = h;
    return CID_OK;
}

void cid_esr_destroy(cid_esr_t h) { delete h; }

const char* cid_esr_last_error(cid_esr_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_esr_param_key(cid_esr_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_esr_set_weight(cid_esr_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_esr_set_bn_eps(cid_esr_t h, int block, int which, double eps) {
    if (!h) return CID_ERR_INVALID;
    return h->set_bn_eps(block >= 0 && block < h->R && (which == 0 || which == 1) ? &h->eps[2 * block + which] : nullptr, eps);
}

int cid_esr_missing_weights(cid_esr_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_esr_packed_weights_bytes(cid_esr_t h) { return h ? h->blob_floats() * sizeof(float) : 0; }

int cid_esr_upload_weights(cid_esr_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, h->blob_floats(), [h](float* b) { esr_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_esr_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    EsrPlan p;
    const int rc = esr_plan(N, H, W, p);
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

int cid_esr_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    EsrPlan p;
    const int rc = esr_plan(N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    if (s == "x1") *offset_bytes = p.x1;
    else if (s == "tail_in") *offset_bytes = p.cur;
    else return CID_ERR_KEY;
    *C = 64;
    *Hs = H;
    *Ws = W;
    *channel_block = 8;
    return CID_OK;
}

int cid_esr_forward(cid_esr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, void* workspace,
                    size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (const int rc = check_image_io(h, "cid_esr_forward", in, in_fmt, out, out_fmt, workspace)) return rc;
    EsrPlan p;
    if (esr_plan(N, H, W, p) != CID_OK) return h->fail(CID_ERR_SHAPE, "cid_esr_forward: input shape not accepted (N, H, W >= 1, H*W < 2^31)");
    if (workspace_bytes < p.total || ((uintptr_t)workspace & 255))
        return h->fail(CID_ERR_WORKSPACE, "cid_esr_forward: workspace smaller than cid_esr_workspace_bytes() or not 256-byte aligned");
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, "cid_esr_forward: weights not uploaded");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, std::string("cid_esr_forward: ") + what + ": " + hipGetErrorString(hipGetLastError())); };
    char* ws = static_cast<char*>(workspace);
    float *x1 = reinterpret_cast<float*>(ws + p.x1), *mid = reinterpret_cast<float*>(ws + p.mid), *cur = reinterpret_cast<float*>(ws + p.cur);
    const float* blob = h->dev_blob;
    const int R = h->R;

    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        const unsigned imgs = (unsigned)std::min(kDiscChunk, N - n0);
        const EsrHeadArgs a{in, x1, R == 0 ? cur : nullptr, blob, H, W, n0};
        const dim3 grid((unsigned)(((long long)H * W + D_THREADS - 1) / D_THREADS), imgs);
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esr_head<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_esr_head<false>, grid, dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("head");
    }
    for (int i = 0; i < R; ++i)
        for (int c = 0; c < 2; ++c)
            for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
                EsrConvArgs a{};
                a.w = blob + kEsrHeadSeg + (size_t)(2 * i + c) * kEsrConvSeg;
                a.H = H;
                a.W = W;
                a.tiles_x = p.ctiles_x;
                a.n0 = n0;
                const dim3 grid((unsigned)p.ctiles, (unsigned)std::min(kDiscChunk, N - n0)), block(D_THREADS);
                if (c == 0) {   // block.0-2: the block's input (x1 for the first block) -> mid
                    a.in = i == 0 ? x1 : cur;
                    a.out = mid;
                    hipLaunchKernelGGL(k_esr_conv<EPI_PRELU>, grid, block, 0, s, a);
                } else {        // block.3-4 and the residual sum -> cur (in place from the second block on)
                    a.in = mid;
                    a.out = cur;
                    a.res = i == 0 ? x1 : cur;
                    a.x1 = x1;
                    if (i == R - 1) hipLaunchKernelGGL(k_esr_conv<EPI_SUM>, grid, block, 0, s, a);
                    else hipLaunchKernelGGL(k_esr_conv<EPI_RES>, grid, block, 0, s, a);
                }
                if (hipPeekAtLastError() != hipSuccess) return herr("trunk");
            }
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        const EsrTailArgs a{cur, out, blob + kEsrHeadSeg + 2 * (size_t)R * kEsrConvSeg, H, W, p.ttiles_x, n0};
        const dim3 grid((unsigned)p.ttiles, (unsigned)std::min(kDiscChunk, N - n0));
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_esr_tail<true>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_esr_tail<false>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("tail");
    }
    return CID_OK;
}

}  // extern "C"

// ---- the server's SRGANGenerator (cid_sr_*): weight staging, BatchNorm folding, workspace plan and launch sequence; kernels in
// srgan_kernels.h (head, upscale stage, tail) and esrgan_kernels.h (trunk) ----
namespace {

constexpr int kSrBlocks = 5;
constexpr size_t kSrUpSeg = (size_t)S_UP_W + 256 + 64;           // weights, bias[256] in packed order, slope (padded to 64)

KeyTable sr_keys(int stages) {
    KeyTable k;
    keys_head9(k);
    for (int i = 0; i < kSrBlocks; ++i) keys_res_block(k, "res_blocks." + std::to_string(i) + ".");
    k.conv("mid.", 64, 64, 3);
    for (int u = 0; u < stages; ++u) {
        k.conv("upscale." + std::to_string(3 * u) + ".", 256, 64, 3);
        k.tensor("upscale." + std::to_string(3 * u + 2) + ".weight", {1});
    }
    k.conv("final.", 3, 64, 9);
    return k;
}

int sr_stages(int scale) { return scale == 1 ? 0 : scale == 2 ? 1 : scale == 4 ? 2 : scale == 8 ? 3 : -1; }

struct SrPlan {
    int stages;
    size_t x0, mid, cur, up[3], total;   // byte offsets of the C8 tensors; `mid` ends as the trunk's result, up[k] is stage k's output
    int ctiles_x, ctiles;                // trunk tiles (16 x 16) of the padded image
};

int sr_plan(int N, int Hp, int Wp, int scale, SrPlan& p) {
    p.stages = sr_stages(scale);
    if (p.stages < 0) return CID_ERR_INVALID;
    if (N < 1 || Hp < 1 || Wp < 1) return CID_ERR_SHAPE;
    if ((long long)Hp * Wp > 0x7fffffffLL / ((long long)scale * scale)) return CID_ERR_SHAPE;   // a pixel index inside one image is an int
    const size_t t = align256((size_t)N * 64 * Hp * Wp * sizeof(float));
    p.x0 = 0;
    p.mid = t;
    p.cur = 2 * t;
    size_t at = 3 * t;
    for (int u = 0; u < p.stages; ++u) {
        p.up[u] = at;
        at += align256((size_t)N * 64 * ((size_t)Hp << (u + 1)) * ((size_t)Wp << (u + 1)) * sizeof(float));
    }
    p.total = at;
    p.ctiles_x = (Wp + D_TW - 1) / D_TW;
    p.ctiles = ((Hp + DiscGeom<64, 64, 1>::TH - 1) / DiscGeom<64, 64, 1>::TH) * p.ctiles_x;
    return CID_OK;
}

}  // namespace

struct cid_sr_s : WeightStore {
    int scale = 1, stages = 0;
    double eps[2 * kSrBlocks];
    // head, ten block convolutions, mid, the upscale stages, tail
    size_t up_off(int u) const { return kEsrHeadSeg + (2 * (size_t)kSrBlocks + 1) * kEsrConvSeg + (size_t)u * kSrUpSeg; }
    size_t tail_off() const { return up_off(stages); }
    size_t blob_floats() const { return tail_off() + kEsrTailSeg; }
};

namespace {
// Upscale stage u: [half][chunk][tap][ci % 8][128 packed columns], the columns in the order of s_up_conv_channel; bias; slope.
void sr_pack_up(const cid_sr_s* h, float* seg, int u) {
    const float* w = h->get("upscale." + std::to_string(3 * u) + ".weight");
    const float* bias = h->get("upscale." + std::to_string(3 * u) + ".bias");
    for (int J = 0; J < 256; ++J) {
        const int cc = s_up_conv_channel(J);
        for (int ci = 0; ci < 64; ++ci)
            for (int tap = 0; tap < 9; ++tap)
                seg[(size_t)(J / 128) * (64 * 9 * 128) + ((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * 128 + J % 128] = w[((size_t)cc * 64 + ci) * 9 + tap];
        seg[S_UP_BIAS + J] = bias[cc];
    }
    seg[S_UP_SLOPE] = h->get("upscale." + std::to_string(3 * u + 2) + ".weight")[0];
}

// The blob from the staged tensors: the head, the ten block convolutions, `mid` with the identity fold (s, t) = (1, 0), the upscale
// stages, the tail.
void sr_pack(const cid_sr_s* h, float* b) {
    pack_head9(*h, b);
    for (int l = 0; l < 2 * kSrBlocks; ++l)
        pack_res_conv(*h, b + kEsrHeadSeg + (size_t)l * kEsrConvSeg, "res_blocks." + std::to_string(l / 2) + ".", l % 2, h->eps[l]);
    float* mid = b + kEsrHeadSeg + 2 * (size_t)kSrBlocks * kEsrConvSeg;   // bias only; fmaf(1, z, 0) = z
    pack_conv64(mid, h->get("mid.weight"), h->get("mid.bias"));
    std::fill(mid + E_CONV_S, mid + E_CONV_S + 64, 1.f);
    for (int u = 0; u < h->stages; ++u) sr_pack_up(h, b + h->up_off(u), u);
    pack_tail9(*h, b + h->tail_off());
}
}  // namespace

extern "C" {

int cid_sr_create(cid_sr_t* out, int scale_factor) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (sr_stages(scale_factor) < 0) return CID_ERR_INVALID;
    cid_sr_s* h = new (std::nothrow) cid_sr_s();
    if (!h) return CID_ERR_INVALID;
    h->scale = scale_factor;
    h->stages = sr_stages(scale_factor);
    h->init("cid_sr", sr_keys(h->stages));
    std::fill(h->eps, h->eps + 2 * kSrBlocks, 1e-5);
    *out = h;
    return CID_OK;
}

void cid_sr_destroy(cid_sr_t h) { delete h; }

const char* cid_sr_last_error(cid_sr_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_sr_param_key(cid_sr_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_sr_set_weight(cid_sr_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_sr_set_bn_eps(cid_sr_t h, int block, int which, double eps) {
    if (!h) return CID_ERR_INVALID;
    return h->set_bn_eps(block >= 0 && block < kSrBlocks && (which == 0 || which == 1) ? &h->eps[2 * block + which] : nullptr, eps);
}

int cid_sr_missing_weights(cid_sr_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_sr_packed_weights_bytes(cid_sr_t h) { return h ? h->blob_floats() * sizeof(float) : 0; }

int cid_sr_upload_weights(cid_sr_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, h->blob_floats(), [h](float* b) { sr_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_sr_workspace_bytes(int N, int Hp, int Wp, int scale_factor, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    SrPlan p;
    const int rc = sr_plan(N, Hp, Wp, scale_factor, p);
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

int cid_sr_stage_view(const char* stage, int N, int Hp, int Wp, int scale_factor, size_t* offset_bytes, int* C, int* Hs, int* Ws,
                      int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    SrPlan p;
    const int rc = sr_plan(N, Hp, Wp, scale_factor, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    int shift = 0;
    if (s == "x0") *offset_bytes = p.x0;
    else if (s == "trunk") *offset_bytes = p.mid;
    else if (s == "up1" && p.stages >= 2) *offset_bytes = p.up[0], shift = 1;
    else if (s == "up2" && p.stages >= 3) *offset_bytes = p.up[1], shift = 2;
    else if (s == "tail_in") *offset_bytes = p.stages ? p.up[p.stages - 1] : p.mid, shift = p.stages;
    else return CID_ERR_KEY;
    *C = 64;
    *Hs = Hp << shift;
    *Ws = Wp << shift;
    *channel_block = 8;
    return CID_OK;
}

int cid_sr_forward(cid_sr_t h, const void* in, int in_fmt, void* out, int out_fmt, int N, int H, int W, int pad_left, int pad_top,
                   int pad_right, int pad_bottom, unsigned flags, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (const int rc = check_image_io(h, "cid_sr_forward", in, in_fmt, out, out_fmt, workspace)) return rc;
    if (flags & ~(unsigned)CID_SR_RAW) return h->fail(CID_ERR_INVALID, "cid_sr_forward: unknown flags");
    if ((flags & CID_SR_RAW) && out_fmt != CID_FMT_F32_NCHW) return h->fail(CID_ERR_INVALID, "cid_sr_forward: CID_SR_RAW needs an fp32 output");
    for (const int pad : {pad_left, pad_top, pad_right, pad_bottom})
        if (pad < 0 || pad > 4096) return h->fail(CID_ERR_INVALID, "cid_sr_forward: pads must lie in [0, 4096]");
    if (N < 1 || H < 1 || W < 1 || H > 0x7fffffff - 8192 || W > 0x7fffffff - 8192)
        return h->fail(CID_ERR_SHAPE, "cid_sr_forward: input shape not accepted (N, H, W >= 1)");
    const int Hp = H + pad_top + pad_bottom, Wp = W + pad_left + pad_right;
    SrPlan p;
    if (sr_plan(N, Hp, Wp, h->scale, p) != CID_OK)
        return h->fail(CID_ERR_SHAPE, "cid_sr_forward: input shape not accepted (scale^2 * Hp * Wp < 2^31)");
    if (workspace_bytes < p.total || ((uintptr_t)workspace & 255))
        return h->fail(CID_ERR_WORKSPACE, "cid_sr_forward: workspace smaller than cid_sr_workspace_bytes() or not 256-byte aligned");
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, "cid_sr_forward: weights not uploaded");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, std::string("cid_sr_forward: ") + what + ": " + hipGetErrorString(hipGetLastError())); };
    char* ws = static_cast<char*>(workspace);
    float *x0 = reinterpret_cast<float*>(ws + p.x0), *mid = reinterpret_cast<float*>(ws + p.mid), *cur = reinterpret_cast<float*>(ws + p.cur);
    const float* blob = h->dev_blob;

    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        const SrHeadArgs a{in, x0, blob, H, W, Hp, Wp, pad_left, pad_top, n0};
        const dim3 grid((unsigned)(((long long)Hp * Wp + D_THREADS - 1) / D_THREADS), (unsigned)std::min(kDiscChunk, N - n0));
        if (in_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_sr_head<true>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_sr_head<false>, grid, dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("head");
    }
    // launches 0 .. 9: the blocks' convolutions (x0 or cur -> mid -> cur); launch 10: mid(cur) + x0 -> mid
    for (int l = 0; l <= 2 * kSrBlocks; ++l)
        for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
            EsrConvArgs a{};
            a.w = blob + kEsrHeadSeg + (size_t)l * kEsrConvSeg;
            a.H = Hp;
            a.W = Wp;
            a.tiles_x = p.ctiles_x;
            a.n0 = n0;
            const dim3 grid((unsigned)p.ctiles, (unsigned)std::min(kDiscChunk, N - n0)), block(D_THREADS);
            if (l == 2 * kSrBlocks) {
                a.in = cur;
                a.out = mid;
                a.res = x0;
                hipLaunchKernelGGL(k_esr_conv<EPI_RES>, grid, block, 0, s, a);
            } else if (l % 2 == 0) {
                a.in = l == 0 ? x0 : cur;
                a.out = mid;
                hipLaunchKernelGGL(k_esr_conv<EPI_PRELU>, grid, block, 0, s, a);
            } else {
                a.in = mid;
                a.out = cur;
                hipLaunchKernelGGL(k_esr_conv<EPI_BN>, grid, block, 0, s, a);
            }
            if (hipPeekAtLastError() != hipSuccess) return herr("trunk");
        }
    const float* u = mid;
    int Hu = Hp, Wu = Wp;
    for (int k = 0; k < p.stages; ++k) {
        float* dst = reinterpret_cast<float*>(ws + p.up[k]);
        const int tiles_x = (Wu + D_TW - 1) / D_TW;
        const int tiles = ((Hu + DiscGeom<64, 128, 1>::TH - 1) / DiscGeom<64, 128, 1>::TH) * tiles_x;
        for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
            const SrUpArgs a{u, dst, blob + h->up_off(k), Hu, Wu, tiles_x, n0};
            const dim3 grid((unsigned)tiles, (unsigned)std::min(kDiscChunk, N - n0), 2);
            hipLaunchKernelGGL(k_sr_up, grid, dim3(D_THREADS), 0, s, a);
            if (hipPeekAtLastError() != hipSuccess) return herr("upscale");
        }
        u = dst;
        Hu *= 2;
        Wu *= 2;
    }
    const int ttiles_x = (Wu + E_TAIL_TW - 1) / E_TAIL_TW;
    const int ttiles = ((Hu + E_TAIL_TH - 1) / E_TAIL_TH) * ttiles_x;
    for (int n0 = 0; n0 < N; n0 += kDiscChunk) {
        const EsrTailArgs a{u, out, blob + h->tail_off(), Hu, Wu, ttiles_x, n0};
        const dim3 grid((unsigned)ttiles, (unsigned)std::min(kDiscChunk, N - n0));
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_sr_tail<SR_OUT_U8>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else if (flags & CID_SR_RAW) hipLaunchKernelGGL(k_sr_tail<SR_OUT_RAW>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_sr_tail<SR_OUT_F32>, grid, dim3(E_TAIL_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("tail");
    }
    return CID_OK;
}

}  // extern "C"

// ---- the server's CGANGenerator (cid_cg_*): weight staging, BatchNorm folding, workspace plan and launch sequence; kernels in
// cgan_kernels.h ----
namespace {

constexpr int kCgMaxClasses = 1 << 20;
constexpr int kCgMaxN = 1 << 18;          // every grid and every int index of the kernels stays below 2^31
const int kCgBn[4] = {0, 3, 6, 9};        // model.<i> of the four BatchNorms
const int kCgUp[3] = {2, 5, 8};           // model.<i> of the three transposed convolutions
const int kCgCin[3] = {128, 128, 64}, kCgCout[3] = {128, 64, 32};

std::string cg_layer(int i) { return "model." + std::to_string(i) + "."; }

KeyTable cg_keys(int n_classes) {
    KeyTable k;
    k.tensor("label_emb.weight", {n_classes, CG_LATENT});
    k.tensor("l1.weight", {CG_FEAT, 2 * CG_LATENT});
    k.tensor("l1.bias", {CG_FEAT});
    k.batchnorm(cg_layer(kCgBn[0]), 128);
    for (int u = 0; u < 3; ++u) {
        k.tensor(cg_layer(kCgUp[u]) + "weight", {kCgCin[u], kCgCout[u], 4, 4});
        k.tensor(cg_layer(kCgUp[u]) + "bias", {kCgCout[u]});
        k.batchnorm(cg_layer(kCgBn[u + 1]), kCgCout[u]);
    }
    k.conv("model.11.", 3, 32, 3);
    return k;
}

size_t cg_align64(size_t floats) { return (floats + 63) & ~(size_t)63; }

struct CgPlan {
    size_t l1, t[3], total;   // byte offsets of the C8 tensors: l1's [N,128,8,8] and the three stages' outputs
};

int cg_plan(int N, CgPlan& p) {
    if (N < 1 || N > kCgMaxN) return CID_ERR_SHAPE;
    size_t at = 0;
    p.l1 = at;
    at += align256((size_t)N * CG_FEAT * sizeof(float));
    for (int u = 0; u < 3; ++u) {
        p.t[u] = at;
        at += align256((size_t)N * kCgCout[u] * (256u << (2 * u)) * sizeof(float));
    }
    p.total = at;
    return CID_OK;
}

}  // namespace

struct cid_cg_s : WeightStore {
    int n_classes = 10;
    double eps[4];
    // the linear, the three stages (weights, bias, s, t), the tail, the embedding table
    size_t up_off(int u) const {
        size_t at = cg_align64(CG_LIN_SEG);
        for (int i = 0; i < u; ++i) at += cg_align64((size_t)16 * kCgCin[i] * kCgCout[i] + 3 * kCgCout[i]);
        return at;
    }
    size_t tail_off() const { return up_off(3); }
    size_t emb_off() const { return tail_off() + CG_TAIL_SEG; }
    size_t blob_floats() const { return emb_off() + cg_align64((size_t)n_classes * CG_LATENT); }
};

namespace {
// The blob from the staged tensors: the kernels' weight layouts, each BatchNorm folded (pack_bn_fold).
void cg_pack(const cid_cg_s* h, float* b) {
    const auto fold = [&](int which, int C, float* s_out, float* t_out) { pack_bn_fold(*h, cg_layer(kCgBn[which]), h->eps[which], C, s_out, t_out); };
    {   // linear: [tile][lane][52]: lane (l16, kq) holds row l16's weights of k = 4 s + kq
        const float *w = h->get("l1.weight"), *bias = h->get("l1.bias");
        for (int tile = 0; tile < CG_LIN_TILES; ++tile)
            for (int row = 0; row < 16; ++row) {
                const int j = cg_lin_feature(tile, row);
                for (int kq = 0; kq < 4; ++kq)
                    for (int s = 0; s < CG_LIN_STEPS; ++s)
                        b[((size_t)tile * 64 + kq * 16 + row) * CG_LIN_LSTR + s] = w[(size_t)j * (2 * CG_LATENT) + 4 * s + kq];
                b[CG_LIN_BIAS + tile * 16 + row] = bias[j];
            }
        fold(0, 128, b + CG_LIN_S, b + CG_LIN_T);
    }
    for (int u = 0; u < 3; ++u) {
        float* seg = b + h->up_off(u);
        const int CI = kCgCin[u], CO = kCgCout[u];
        const float* w = h->get(cg_layer(kCgUp[u]) + "weight");
        for (int ci = 0; ci < CI; ++ci)
            for (int co = 0; co < CO; ++co)
                for (int ky = 0; ky < 4; ++ky)
                    for (int kx = 0; kx < 4; ++kx) seg[cg_up_windex(CO, ci, co, ky, kx)] = w[(((size_t)ci * CO + co) * 4 + ky) * 4 + kx];
        float* tail = seg + (size_t)16 * CI * CO;
        std::memcpy(tail, h->get(cg_layer(kCgUp[u]) + "bias"), CO * sizeof(float));
        fold(u + 1, CO, tail + CO, tail + 2 * CO);
    }
    {   // tail: [ci][tap][co], then the biases
        float* seg = b + h->tail_off();
        const float* w = h->get("model.11.weight");
        for (int co = 0; co < 3; ++co)
            for (int ci = 0; ci < 32; ++ci)
                for (int tap = 0; tap < 9; ++tap) seg[(ci * 9 + tap) * 3 + co] = w[((size_t)co * 32 + ci) * 9 + tap];
        std::memcpy(seg + CG_TAIL_W, h->get("model.11.bias"), 3 * sizeof(float));
    }
    std::memcpy(b + h->emb_off(), h->get("label_emb.weight"), (size_t)h->n_classes * CG_LATENT * sizeof(float));
}
}  // namespace

extern "C" {

int cid_cg_create(cid_cg_t* out, int n_classes) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    if (n_classes < 1 || n_classes > kCgMaxClasses) return CID_ERR_INVALID;
    cid_cg_s* h = new (std::nothrow) cid_cg_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_cg", cg_keys(n_classes));
    h->n_classes = n_classes;
    std::fill(h->eps, h->eps + 4, 1e-5);
    *out = h;
    return CID_OK;
}

void cid_cg_destroy(cid_cg_t h) { delete h; }

const char* cid_cg_last_error(cid_cg_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_cg_param_key(cid_cg_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_cg_set_weight(cid_cg_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_cg_set_bn_eps(cid_cg_t h, int which, double eps) {
    return h ? h->set_bn_eps(which >= 0 && which <= 3 ? &h->eps[which] : nullptr, eps) : CID_ERR_INVALID;
}

int cid_cg_missing_weights(cid_cg_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_cg_packed_weights_bytes(cid_cg_t h) { return h ? h->blob_floats() * sizeof(float) : 0; }

int cid_cg_upload_weights(cid_cg_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, h->blob_floats(), [h](float* b) { cg_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_cg_workspace_bytes(int N, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    CgPlan p;
    const int rc = cg_plan(N, p);
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

int cid_cg_stage_view(const char* stage, int N, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    CgPlan p;
    const int rc = cg_plan(N, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    int u = -1;
    if (s == "l1") *offset_bytes = p.l1;
    else if (s == "t1") u = 0;
    else if (s == "t2") u = 1;
    else if (s == "t3") u = 2;
    else return CID_ERR_KEY;
    if (u >= 0) *offset_bytes = p.t[u];
    *C = u < 0 ? 128 : kCgCout[u];
    *Hs = *Ws = u < 0 ? 8 : 16 << u;
    *channel_block = 8;
    return CID_OK;
}

int cid_cg_latent(uint64_t seed, uint64_t first_index, int N, float* z_out, void* stream) {
    if (!z_out || ((uintptr_t)z_out & 3)) return CID_ERR_INVALID;
    if (N < 1 || N > kCgMaxN) return CID_ERR_SHAPE;
    const CgLatentArgs a{z_out, (long long)N * CG_LATENT, seed + first_index};
    hipLaunchKernelGGL(k_cg_latent, dim3((unsigned)((a.count + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, static_cast<hipStream_t>(stream), a);
    return hipPeekAtLastError() == hipSuccess ? CID_OK : CID_ERR_HIP;
}

int cid_cg_forward(cid_cg_t h, const float* z, const int64_t* labels, void* out, int out_fmt, int N, unsigned flags, void* workspace,
                   size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!z || !labels || !out || !workspace) return h->fail(CID_ERR_INVALID, "cid_cg_forward: null pointer");
    if (out_fmt != CID_FMT_F32_NCHW && out_fmt != CID_FMT_U8_NHWC) return h->fail(CID_ERR_INVALID, "cid_cg_forward: unknown format");
    if (((uintptr_t)z & 3) || ((uintptr_t)labels & 7) || (out_fmt == CID_FMT_F32_NCHW && ((uintptr_t)out & 3)))
        return h->fail(CID_ERR_INVALID, "cid_cg_forward: misaligned operand");
    if (flags & ~(unsigned)CID_CG_RAW) return h->fail(CID_ERR_INVALID, "cid_cg_forward: unknown flags");
    if ((flags & CID_CG_RAW) && out_fmt != CID_FMT_F32_NCHW) return h->fail(CID_ERR_INVALID, "cid_cg_forward: CID_CG_RAW needs an fp32 output");
    CgPlan p;
    if (cg_plan(N, p) != CID_OK) return h->fail(CID_ERR_SHAPE, "cid_cg_forward: batch size not accepted (1 <= N <= 2^18)");
    if (workspace_bytes < p.total || ((uintptr_t)workspace & 255))
        return h->fail(CID_ERR_WORKSPACE, "cid_cg_forward: workspace smaller than cid_cg_workspace_bytes() or not 256-byte aligned");
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, "cid_cg_forward: weights not uploaded");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, std::string("cid_cg_forward: ") + what + ": " + hipGetErrorString(hipGetLastError())); };
    char* ws = static_cast<char*>(workspace);
    const float* blob = h->dev_blob;
    float* l1 = reinterpret_cast<float*>(ws + p.l1);
    float* t[3] = {reinterpret_cast<float*>(ws + p.t[0]), reinterpret_cast<float*>(ws + p.t[1]), reinterpret_cast<float*>(ws + p.t[2])};

    {
        const CgLinearArgs a{z, reinterpret_cast<const long long*>(labels), l1, blob, blob + h->emb_off(), N, h->n_classes};
        hipLaunchKernelGGL(k_cg_linear, dim3(CG_LIN_TILES), dim3(64), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("linear");
    }
    {
        const CgUpArgs a{l1, t[0], blob + h->up_off(0)};
        hipLaunchKernelGGL((k_cg_up<128, 128, 8>), dim3((unsigned)N * CgUpGeom<128, 128, 8>::TILES), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("up 1");
    }
    {
        const CgUpArgs a{t[0], t[1], blob + h->up_off(1)};
        hipLaunchKernelGGL((k_cg_up<128, 64, 16>), dim3((unsigned)N * CgUpGeom<128, 64, 16>::TILES), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("up 2");
    }
    {
        const CgUpArgs a{t[1], t[2], blob + h->up_off(2)};
        hipLaunchKernelGGL((k_cg_up<64, 32, 32>), dim3((unsigned)N * CgUpGeom<64, 32, 32>::TILES), dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("up 3");
    }
    {
        const CgTailArgs a{t[2], out, blob + h->tail_off(), (long long)N * 4096};
        const dim3 grid((unsigned)(a.count / D_THREADS));
        if (out_fmt == CID_FMT_U8_NHWC) hipLaunchKernelGGL(k_cg_tail<CG_OUT_U8>, grid, dim3(D_THREADS), 0, s, a);
        else if (flags & CID_CG_RAW) hipLaunchKernelGGL(k_cg_tail<CG_OUT_RAW>, grid, dim3(D_THREADS), 0, s, a);
        else hipLaunchKernelGGL(k_cg_tail<CG_OUT_F32>, grid, dim3(D_THREADS), 0, s, a);
        if (hipPeekAtLastError() != hipSuccess) return herr("tail");
    }
    return CID_OK;
}

}  // extern "C"

// ---- LPIPS(net='alex') (cid_lpips_*): weight staging, workspace plan and launch sequence; kernels in lpips_kernels.h ----
namespace {

constexpr int kLpMaxN = 1 << 20;
constexpr int kLpMinSide = 31;
const int kLpSlice[5] = {0, 3, 6, 8, 10};            // net.slice<k+1>.<i>
const int kLpCin[5] = {3, 64, 192, 384, 256}, kLpKs[5] = {11, 5, 3, 3, 3};

// scaling_layer.* ahead of a tower's convolutions, lin<k>.* behind them: the layout LPIPS and the VGG tower share
void keys_scaling(KeyTable& k) {
    k.tensor("scaling_layer.shift", {1, 3, 1, 1});
    k.tensor("scaling_layer.scale", {1, 3, 1, 1});
}
std::string lp_lin_name(int l) { return "lin" + std::to_string(l) + ".model.1.weight"; }
std::string lp_conv_name(int l) { return "net.slice" + std::to_string(l + 1) + "." + std::to_string(kLpSlice[l]) + "."; }

const KeyTable& lp_key_table() {
    static const KeyTable table = [] {
        KeyTable k;
        keys_scaling(k);
        for (int l = 0; l < LP_TAPS; ++l) k.conv(lp_conv_name(l), lp_channels(l), kLpCin[l], kLpKs[l]);
        for (int l = 0; l < LP_TAPS; ++l) k.tensor(lp_lin_name(l), {1, lp_channels(l), 1, 1});
        return k;
    }();
    return table;
}

// blob segments (floats, 64-float aligned): the head, relu2 ... relu5 (packed weights then biases), the five lin vectors
size_t lp_conv_off(int l) {   // l = 1 .. 4; l = 5: the lin segment
    size_t at = LP_HEAD_SEG;
    for (int i = 1; i < l; ++i) at += cg_align64((size_t)lp_channels(i) * kLpCin[i] * kLpKs[i] * kLpKs[i] + lp_channels(i));
    return at;
}
size_t lp_blob_floats() { return lp_conv_off(5) + LP_LIN_SEG; }

struct LpPlan {
    int Hs[LP_TAPS], Ws[LP_TAPS];   // sizes of relu1 ... relu5
    size_t tap[LP_TAPS], total;     // byte offsets of the C8 tensors (2 N images each)
};

int lp_plan(int N, int H, int W, LpPlan& p) {
    if (N < 1 || N > kLpMaxN || H < kLpMinSide || W < kLpMinSide || (long long)H * W >= (1ll << 31)) return CID_ERR_SHAPE;
    p.Hs[0] = (H - 7) / 4 + 1, p.Ws[0] = (W - 7) / 4 + 1;
    p.Hs[1] = (p.Hs[0] - 3) / 2 + 1, p.Ws[1] = (p.Ws[0] - 3) / 2 + 1;
    p.Hs[2] = (p.Hs[1] - 3) / 2 + 1, p.Ws[2] = (p.Ws[1] - 3) / 2 + 1;
    p.Hs[3] = p.Hs[4] = p.Hs[2], p.Ws[3] = p.Ws[4] = p.Ws[2];
    // what a workgroup of the GEMM kernel stages must fit its LDS planes
    if (lp_stage_bound(p.Hs[1], p.Ws[1], 2) > LP_XPOS || lp_stage_bound(p.Hs[2], p.Ws[2], 1) > LP_XPOS) return CID_ERR_SHAPE;
    size_t at = 0;
    for (int k = 0; k < LP_TAPS; ++k) {
        p.tap[k] = at;
        at += align256((size_t)2 * N * lp_channels(k) * p.Hs[k] * p.Ws[k] * sizeof(float));
    }
    p.total = at;
    return CID_OK;
}

}  // namespace

struct cid_lpips_s : WeightStore {};

namespace {
// A tower's head segment: [k][64], bias, and (scaled) the scaling layer's shift and scale
void lp_pack_head(const WeightStore& w, float* b, const std::string& conv, int K, int bias_at, int ss_at, bool scaled) {
    pack_k64(b, w.get(conv + "weight"), K);
    std::memcpy(b + bias_at, w.get(conv + "bias"), 64 * sizeof(float));
    if (!scaled) return;
    std::memcpy(b + ss_at, w.get("scaling_layer.shift"), 3 * sizeof(float));
    std::memcpy(b + ss_at + 4, w.get("scaling_layer.scale"), 3 * sizeof(float));
}

void lp_pack(const cid_lpips_s* h, float* b) {
    lp_pack_head(*h, b, lp_conv_name(0), LP_HEAD_K, LP_HEAD_B, LP_HEAD_SS, true);
    for (int l = 1; l < LP_TAPS; ++l) {
        float* seg = b + lp_conv_off(l);
        const int CO = lp_channels(l), CI = kLpCin[l], KS = kLpKs[l];
        const float* w = h->get(lp_conv_name(l) + "weight");
        for (int co = 0; co < CO; ++co)
            for (int ci = 0; ci < CI; ++ci)
                for (int kh = 0; kh < KS; ++kh)
                    for (int kw = 0; kw < KS; ++kw) seg[lp_conv_windex(CI, KS, co, ci, kh, kw)] = w[(((size_t)co * CI + ci) * KS + kh) * KS + kw];
        std::memcpy(seg + (size_t)CO * CI * KS * KS, h->get(lp_conv_name(l) + "bias"), CO * sizeof(float));
    }
    for (int l = 0; l < LP_TAPS; ++l) std::memcpy(b + lp_conv_off(5) + lp_lin_off(l), h->get(lp_lin_name(l)), lp_channels(l) * sizeof(float));
}

template <int CIN, int COUT, int KS, bool POOL>
void lp_conv_launch(const float* in, float* out, const float* w, int N, int Hs, int Ws, int Ho, int Wo, hipStream_t s) {
    const LpConvArgs a{in, out, w, (long long)2 * N * Ho * Wo, Hs, Ws, Ho, Wo};
    const dim3 grid((unsigned)((a.total + LP_NT - 1) / LP_NT), COUT / LP_MT);
    hipLaunchKernelGGL((k_lpips_conv<CIN, COUT, KS, POOL>), grid, dim3(D_THREADS), 0, s, a);
}
}  // namespace

extern "C" {

int cid_lpips_create(cid_lpips_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    cid_lpips_s* h = new (std::nothrow) cid_lpips_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_lpips", lp_key_table());
    *out = h;
    return CID_OK;
}

void cid_lpips_destroy(cid_lpips_t h) { delete h; }

const char* cid_lpips_last_error(cid_lpips_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_lpips_param_key(cid_lpips_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_lpips_set_weight(cid_lpips_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_lpips_missing_weights(cid_lpips_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_lpips_packed_weights_bytes(cid_lpips_t h) { return h ? lp_blob_floats() * sizeof(float) : 0; }

int cid_lpips_upload_weights(cid_lpips_t h, void* device_blob, void* stream) {
    return h ? h->upload(device_blob, stream, lp_blob_floats(), [h](float* b) { lp_pack(h, b); }) : CID_ERR_INVALID;
}

int cid_lpips_workspace_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    LpPlan p;
    const int rc = lp_plan(N, H, W, p);
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

int cid_lpips_stage_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    LpPlan p;
    const int rc = lp_plan(N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    if (s.size() != 5 || s.compare(0, 4, "relu") != 0 || s[4] < '1' || s[4] > '5') return CID_ERR_KEY;
    const int k = s[4] - '1';
    *offset_bytes = p.tap[k];
    *C = lp_channels(k);
    *Hs = p.Hs[k];
    *Ws = p.Ws[k];
    *channel_block = 8;
    return CID_OK;
}

int cid_lpips(cid_lpips_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
              double* layers, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!a || !b || !out || !workspace) return h->fail(CID_ERR_INVALID, "cid_lpips: null pointer");
    if ((fmt_a != CID_FMT_F32_NCHW && fmt_a != CID_FMT_U8_NHWC) || (fmt_b != CID_FMT_F32_NCHW && fmt_b != CID_FMT_U8_NHWC))
        return h->fail(CID_ERR_INVALID, "cid_lpips: unknown format");
    if ((fmt_a == CID_FMT_F32_NCHW && ((uintptr_t)a & 3)) || (fmt_b == CID_FMT_F32_NCHW && ((uintptr_t)b & 3)) || ((uintptr_t)out & 7) ||
        ((uintptr_t)layers & 7))
        return h->fail(CID_ERR_INVALID, "cid_lpips: misaligned operand");
    if (flags & ~(unsigned)CID_LPIPS_UNIT_VIEW) return h->fail(CID_ERR_INVALID, "cid_lpips: unknown flags");
    LpPlan p;
    if (lp_plan(N, H, W, p) != CID_OK)
        return h->fail(CID_ERR_SHAPE, "cid_lpips: shape not accepted (1 <= N <= 2^20, H and W >= 31 and within the kernels' tile limit)");
    if (workspace_bytes < p.total || ((uintptr_t)workspace & 255))
        return h->fail(CID_ERR_WORKSPACE, "cid_lpips: workspace smaller than cid_lpips_workspace_bytes() or not 256-byte aligned");
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, "cid_lpips: weights not uploaded");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, std::string("cid_lpips: ") + what + ": " + hipGetErrorString(hipGetLastError())); };
    char* ws = static_cast<char*>(workspace);
    const float* blob = h->dev_blob;
    float* t[LP_TAPS];
    for (int k = 0; k < LP_TAPS; ++k) t[k] = reinterpret_cast<float*>(ws + p.tap[k]);

    for (long long n0 = 0; n0 < 2ll * N; n0 += kDiscChunk) {
        const LpHeadArgs ha{a, b, t[0], blob, H, W, p.Hs[0], p.Ws[0], N, (int)n0, fmt_a == CID_FMT_U8_NHWC, fmt_b == CID_FMT_U8_NHWC,
                            (flags & CID_LPIPS_UNIT_VIEW) != 0};
        const dim3 grid((unsigned)((p.Hs[0] * p.Ws[0] + LP_HEAD_PIX - 1) / LP_HEAD_PIX), (unsigned)std::min<long long>(kDiscChunk, 2ll * N - n0));
        hipLaunchKernelGGL(k_lpips_head, grid, dim3(LP_HEAD_PIX), 0, s, ha);
        if (hipPeekAtLastError() != hipSuccess) return herr("head");
    }
    lp_conv_launch<64, 192, 5, true>(t[0], t[1], blob + lp_conv_off(1), N, p.Hs[0], p.Ws[0], p.Hs[1], p.Ws[1], s);
    if (hipPeekAtLastError() != hipSuccess) return herr("relu2");
    lp_conv_launch<192, 384, 3, true>(t[1], t[2], blob + lp_conv_off(2), N, p.Hs[1], p.Ws[1], p.Hs[2], p.Ws[2], s);
    if (hipPeekAtLastError() != hipSuccess) return herr("relu3");
    lp_conv_launch<384, 256, 3, false>(t[2], t[3], blob + lp_conv_off(3), N, p.Hs[2], p.Ws[2], p.Hs[3], p.Ws[3], s);
    if (hipPeekAtLastError() != hipSuccess) return herr("relu4");
    lp_conv_launch<256, 256, 3, false>(t[3], t[4], blob + lp_conv_off(4), N, p.Hs[3], p.Ws[3], p.Hs[4], p.Ws[4], s);
    if (hipPeekAtLastError() != hipSuccess) return herr("relu5");
    {
        LpDistArgs da;
        for (int k = 0; k < LP_TAPS; ++k) {
            da.tap[k] = t[k];
            da.P[k] = p.Hs[k] * p.Ws[k];
        }
        da.lin = blob + lp_conv_off(5);
        da.out = out;
        da.layers = layers;
        da.N = N;
        hipLaunchKernelGGL(k_lpips_dist<LpAlexTaps>, dim3((unsigned)N), dim3(D_THREADS), 0, s, da);
        if (hipPeekAtLastError() != hipSuccess) return herr("distance");
    }
    return CID_OK;
}

}  // extern "C"

// ---- VGG16 features (cid_vgg_*): LPIPS(net='vgg') and the content loss; kernels in vgg_kernels.h and lpips_kernels.h ----
namespace {

static_assert(VG_MAX_SIDE == CID_VGG_MAX_SIDE, "vgg_kernels.h and cid.h agree on the largest side");
constexpr int kVgMinSide[2] = {16, 4};               // by form: CID_VGG_LPIPS, CID_VGG_CONTENT
const int kVgIdx[VG_CONVS] = {0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28};   // torchvision's features indices
const int kVgSlice[VG_CONVS] = {1, 1, 2, 2, 3, 3, 3, 4, 4, 4, 5, 5, 5};
const int kVgCin[VG_CONVS] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
const int kVgCout[VG_CONVS] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kVgContentConvs = 7;                   // slice1 ... slice3

std::string vg_conv_name(int l) { return "net.slice" + std::to_string(kVgSlice[l]) + "." + std::to_string(kVgIdx[l]) + "."; }

const KeyTable& vg_key_table() {
    static const KeyTable table = [] {
        KeyTable k;
        keys_scaling(k);
        for (int l = 0; l < VG_CONVS; ++l) k.conv(vg_conv_name(l), kVgCout[l], kVgCin[l], 3);
        for (int l = 0; l < LP_TAPS; ++l) k.tensor(lp_lin_name(l), {1, VgTaps::channels(l), 1, 1});
        return k;
    }();
    return table;
}

// blob segments (floats, 64-float aligned): the head, convolutions 1 ... 12 (packed weights then biases), the five lin vectors
size_t vg_conv_off(int l) {   // l = 1 .. 12; l = 13: the lin segment
    size_t at = VG_HEAD_SEG;
    for (int i = 1; i < l; ++i) at += cg_align64((size_t)kVgCout[i] * kVgCin[i] * 9 + kVgCout[i]);
    return at;
}
size_t vg_blob_floats() { return vg_conv_off(VG_CONVS) + VG_LIN_SEG; }

struct VgPlan {
    int Hs[LP_TAPS], Ws[LP_TAPS];    // sizes of relu1_2, relu2_2, relu3_3, relu4_3, relu5_3
    size_t s0, s1;                   // byte offsets of the two scratch tensors (the convolutions between the taps)
    size_t tap[LP_TAPS], total;      // byte offsets of the taps (C8, 2 N images each); the content form has the first three
};

int vg_plan(int what, int N, int H, int W, VgPlan& p) {
    if (what != CID_VGG_LPIPS && what != CID_VGG_CONTENT) return CID_ERR_INVALID;
    if (N < 1 || N > kLpMaxN || H < kVgMinSide[what] || W < kVgMinSide[what] || H > VG_MAX_SIDE || W > VG_MAX_SIDE) return CID_ERR_SHAPE;
    // the head's grid.x runs over the whole batch's pixels
    if (((long long)2 * N * H * W + VG_HEAD_PIX - 1) / VG_HEAD_PIX > 0x7fffffffll) return CID_ERR_SHAPE;
    const int taps = what == CID_VGG_LPIPS ? LP_TAPS : 3;
    p.Hs[0] = H, p.Ws[0] = W;
    for (int k = 1; k < LP_TAPS; ++k) p.Hs[k] = p.Hs[k - 1] / 2, p.Ws[k] = p.Ws[k - 1] / 2;
    for (int k = 0; k < taps; ++k)
        if (vg_stage_bound(p.Hs[k], p.Ws[k]) > (k < 1 ? VG_XPOS_WIDE : LP_XPOS)) return CID_ERR_SHAPE;   // cannot happen up to VG_MAX_SIDE
    size_t at = 0;
    p.s0 = at;
    at += align256((size_t)2 * N * 64 * H * W * sizeof(float));
    p.s1 = at;
    at += align256((size_t)2 * N * 256 * p.Hs[2] * p.Ws[2] * sizeof(float));
    for (int k = 0; k < LP_TAPS; ++k) {
        p.tap[k] = at;
        if (k < taps) at += align256((size_t)2 * N * VgTaps::channels(k) * p.Hs[k] * p.Ws[k] * sizeof(float));
    }
    p.total = at;
    return CID_OK;
}

// The per-call arena of cid_vgg_content_loss_saved / cid_vgg_content_backward: the seven activations of both towers (2 N images),
// then the seven gradient tensors of tower a (N images), in backward order.
constexpr int kVgSaved = 7;
const char* const kVgActName[kVgSaved] = {"relu1_1", "relu1_2", "relu2_1", "relu2_2", "relu3_1", "relu3_2", "relu3_3"};
const int kVgActLevel[kVgSaved] = {0, 0, 1, 1, 2, 2, 2};
const char* const kVgGradName[kVgSaved] = {"grad3_3", "grad3_2", "grad3_1", "gradpool2", "grad2_1", "gradpool1", "grad1_1"};
const int kVgGradLevel[kVgSaved] = {2, 2, 2, 2, 1, 1, 0};       // the map size: Hs[level] x Ws[level]
const int kVgGradC[kVgSaved] = {256, 256, 256, 128, 128, 64, 64};

struct VgSavedPlan {
    int Hs[3], Ws[3];
    size_t act[kVgSaved], grad[kVgSaved], total;
};

int vg_saved_plan(int N, int H, int W, VgSavedPlan& p) {
    VgPlan f;
    const int rc = vg_plan(CID_VGG_CONTENT, N, H, W, f);
    if (rc != CID_OK) return rc;
    for (int k = 0; k < 3; ++k) p.Hs[k] = f.Hs[k], p.Ws[k] = f.Ws[k];
    size_t at = 0;
    for (int i = 0; i < kVgSaved; ++i) {
        const int k = kVgActLevel[i];
        p.act[i] = at;
        at += align256((size_t)2 * N * VgTaps::channels(k) * p.Hs[k] * p.Ws[k] * sizeof(float));
    }
    for (int i = 0; i < kVgSaved; ++i) {
        const int k = kVgGradLevel[i];
        p.grad[i] = at;
        at += align256((size_t)N * kVgGradC[i] * p.Hs[k] * p.Ws[k] * sizeof(float));
    }
    p.total = at;
    return CID_OK;
}

// the backward blob (floats): the head's segment, then the data-gradient weights of convolutions 1 ... 6
size_t vg_bwd_off(int l) {   // l = 1 .. 6; l = 7: the end
    size_t at = VG_HEADB_SEG;
    for (int i = 1; i < l; ++i) at += (size_t)kVgCout[i] * kVgCin[i] * 9;
    return at;
}
size_t vg_bwd_floats() { return vg_bwd_off(kVgContentConvs); }

}  // namespace

struct cid_vgg_s : WeightStore {
    bool full = false;   // the uploaded blob holds all 33 tensors (else slice1 ... slice3 only)
    std::vector<float> bwd_staging;      // the backward blob's staging copy
    const float* dev_bwd = nullptr;      // the uploaded backward blob; dropped when the forward blob is uploaded again
};

namespace {
void vg_pack(const cid_vgg_s* h, float* b, bool full) {
    lp_pack_head(*h, b, vg_conv_name(0), VG_HEAD_K, VG_HEAD_B, VG_HEAD_SS, full);
    for (int l = 1; l < (full ? VG_CONVS : kVgContentConvs); ++l) {
        float* seg = b + vg_conv_off(l);
        const int CO = kVgCout[l], CI = kVgCin[l];
        const float* w = h->get(vg_conv_name(l) + "weight");
        for (int co = 0; co < CO; ++co)
            for (int ci = 0; ci < CI; ++ci)
                for (int t = 0; t < 9; ++t) seg[lp_conv_windex(CI, 3, co, ci, t / 3, t % 3)] = w[((size_t)co * CI + ci) * 9 + t];
        std::memcpy(seg + (size_t)CO * CI * 9, h->get(vg_conv_name(l) + "bias"), CO * sizeof(float));
    }
    if (full)
        for (int l = 0; l < LP_TAPS; ++l)
            std::memcpy(b + vg_conv_off(VG_CONVS) + VgTaps::lin_off(l), h->get(lp_lin_name(l)), VgTaps::channels(l) * sizeof(float));
}

// The data gradient of a 3x3, pad-1, stride-1 convolution is a 3x3 convolution with the channel axes swapped and the taps flipped:
// w'[ci][co][kh][kw] = w[co][ci][2 - kh][2 - kw], packed with lp_conv_windex like a forward convolution of co -> ci channels.
void vg_pack_backward(const cid_vgg_s* h, float* b) {
    const float* w0 = h->get(vg_conv_name(0) + "weight");
    for (int t = 0; t < 9; ++t)
        for (int co = 0; co < 64; ++co)
            for (int ci = 0; ci < 3; ++ci) b[(t * 64 + co) * 3 + ci] = w0[(co * 3 + ci) * 9 + (2 - t / 3) * 3 + (2 - t % 3)];
    for (int l = 1; l < kVgContentConvs; ++l) {
        float* seg = b + vg_bwd_off(l);
        const int CG = kVgCout[l], CX = kVgCin[l];
        const float* w = h->get(vg_conv_name(l) + "weight");
        for (int cx = 0; cx < CX; ++cx)
            for (int cg = 0; cg < CG; ++cg)
                for (int t = 0; t < 9; ++t) seg[lp_conv_windex(CG, 3, cx, cg, t / 3, t % 3)] = w[((size_t)cg * CX + cx) * 9 + (8 - t)];
    }
}

// One trunk convolution from an Hs x Ws tensor; the plane size follows the output map's width.  Only the launch that can meet a
// map wider than 339 (relu1_2, at the image's own size) has a wide instantiation.
template <int CIN, int COUT, bool POOL, bool CAN_BE_WIDE>
void vg_conv_launch(const float* in, float* out, const float* w, int N, int Hs, int Ws, hipStream_t s) {
    const int Ho = POOL ? Hs / 2 : Hs, Wo = POOL ? Ws / 2 : Ws;
    const LpConvArgs a{in, out, w, (long long)2 * N * Ho * Wo, Hs, Ws, Ho, Wo};
    const dim3 grid((unsigned)((a.total + LP_NT - 1) / LP_NT), COUT / LP_MT);
    if (vg_stage_bound(Ho, Wo) <= LP_XPOS) {
        hipLaunchKernelGGL((k_lpips_conv<CIN, COUT, 3, POOL, 2, LP_XPOS>), grid, dim3(D_THREADS), 0, s, a);
    } else if constexpr (CAN_BE_WIDE) {
        hipLaunchKernelGGL((k_lpips_conv<CIN, COUT, 3, POOL, 2, VG_XPOS_WIDE>), grid, dim3(D_THREADS), 0, s, a);
    }
}

// the checks cid_vgg_lpips and cid_vgg_content_loss share
int vg_check(cid_vgg_t h, const char* fn, int what, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags,
             const void* out, const void* layers, const void* workspace, size_t workspace_bytes, VgPlan& p, bool saved = false) {
    const std::string f(fn);
    if (!a || !b || !out || !workspace) return h->fail(CID_ERR_INVALID, f + ": null pointer");
    if ((fmt_a != CID_FMT_F32_NCHW && fmt_a != CID_FMT_U8_NHWC) || (fmt_b != CID_FMT_F32_NCHW && fmt_b != CID_FMT_U8_NHWC))
        return h->fail(CID_ERR_INVALID, f + ": unknown format");
    if (saved && fmt_a != CID_FMT_F32_NCHW) return h->fail(CID_ERR_INVALID, f + ": operand a must be fp32 (a uint8 image has no gradient)");
    if ((fmt_a == CID_FMT_F32_NCHW && ((uintptr_t)a & 3)) || (fmt_b == CID_FMT_F32_NCHW && ((uintptr_t)b & 3)) || ((uintptr_t)out & 7) ||
        ((uintptr_t)layers & 7))
        return h->fail(CID_ERR_INVALID, f + ": misaligned operand");
    if (flags & ~(unsigned)CID_LPIPS_UNIT_VIEW) return h->fail(CID_ERR_INVALID, f + ": unknown flags");
    if (vg_plan(what, N, H, W, p) != CID_OK)
        return h->fail(CID_ERR_SHAPE, f + ": shape not accepted (1 <= N <= 2^20, " + std::to_string(kVgMinSide[what]) + " <= H, W <= " +
                                            std::to_string(VG_MAX_SIDE) + ", 2 N H W < 2^37)");
    VgSavedPlan sp;
    if (saved) vg_saved_plan(N, H, W, sp);
    if (workspace_bytes < (saved ? sp.total : p.total) || ((uintptr_t)workspace & 255))
        return h->fail(CID_ERR_WORKSPACE, f + (saved ? ": saved arena smaller than cid_vgg_saved_bytes() or not 256-byte aligned"
                                                     : ": workspace smaller than cid_vgg_workspace_bytes() or not 256-byte aligned"));
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, f + ": weights not uploaded");
    if (what == CID_VGG_LPIPS && !h->full) return h->fail(CID_ERR_STATE, f + ": the handle holds slice1 ... slice3 only (content loss)");
    return CID_OK;
}

// Head and trunk up to convolution `convs` (7: relu3_3, 13: relu5_3); convolution l writes t[l], every tensor C8 with 2 N images, and
// Hs / Ws are the sizes by level (the image's, then one halving per pool).  The plain calls pass their two scratch tensors and the
// taps, the saved call seven tensors of its arena: the same kernels on the same operands, so the same bits.  Returns the name of the
// launch that failed, or null.
const char* vg_features(cid_vgg_t h, float* const* t, const int* Hs, const int* Ws, const void* a, int fmt_a, const void* b, int fmt_b, int N,
                        int H, int W, bool unit, bool scaled, int convs, hipStream_t s) {
    const float* blob = h->dev_blob;
    const auto bad = [] { return hipPeekAtLastError() != hipSuccess; };
    {
        const VgHeadArgs ha{a, b, t[0], blob, (long long)2 * N * H * W, H, W, N, fmt_a == CID_FMT_U8_NHWC, fmt_b == CID_FMT_U8_NHWC, unit, scaled};
        hipLaunchKernelGGL(k_vgg_head, dim3((unsigned)((ha.total + VG_HEAD_PIX - 1) / VG_HEAD_PIX)), dim3(VG_HEAD_PIX), 0, s, ha);
        if (bad()) return "relu1_1";
    }
    vg_conv_launch<64, 64, false, true>(t[0], t[1], blob + vg_conv_off(1), N, Hs[0], Ws[0], s);
    if (bad()) return "relu1_2";
    vg_conv_launch<64, 128, true, false>(t[1], t[2], blob + vg_conv_off(2), N, Hs[0], Ws[0], s);
    if (bad()) return "relu2_1";
    vg_conv_launch<128, 128, false, false>(t[2], t[3], blob + vg_conv_off(3), N, Hs[1], Ws[1], s);
    if (bad()) return "relu2_2";
    vg_conv_launch<128, 256, true, false>(t[3], t[4], blob + vg_conv_off(4), N, Hs[1], Ws[1], s);
    if (bad()) return "relu3_1";
    vg_conv_launch<256, 256, false, false>(t[4], t[5], blob + vg_conv_off(5), N, Hs[2], Ws[2], s);
    if (bad()) return "relu3_2";
    vg_conv_launch<256, 256, false, false>(t[5], t[6], blob + vg_conv_off(6), N, Hs[2], Ws[2], s);
    if (bad()) return "relu3_3";
    if (convs == kVgContentConvs) return nullptr;
    vg_conv_launch<256, 512, true, false>(t[6], t[7], blob + vg_conv_off(7), N, Hs[2], Ws[2], s);
    if (bad()) return "relu4_1";
    vg_conv_launch<512, 512, false, false>(t[7], t[8], blob + vg_conv_off(8), N, Hs[3], Ws[3], s);
    if (bad()) return "relu4_2";
    vg_conv_launch<512, 512, false, false>(t[8], t[9], blob + vg_conv_off(9), N, Hs[3], Ws[3], s);
    if (bad()) return "relu4_3";
    vg_conv_launch<512, 512, true, false>(t[9], t[10], blob + vg_conv_off(10), N, Hs[3], Ws[3], s);
    if (bad()) return "relu5_1";
    vg_conv_launch<512, 512, false, false>(t[10], t[11], blob + vg_conv_off(11), N, Hs[4], Ws[4], s);
    if (bad()) return "relu5_2";
    vg_conv_launch<512, 512, false, false>(t[11], t[12], blob + vg_conv_off(12), N, Hs[4], Ws[4], s);
    if (bad()) return "relu5_3";
    return nullptr;
}

// the plain calls' tensors by convolution: the two scratch tensors between the taps
void vg_plain_tensors(const VgPlan& p, char* ws, float** t) {
    float *s0 = reinterpret_cast<float*>(ws + p.s0), *s1 = reinterpret_cast<float*>(ws + p.s1), *tap[LP_TAPS];
    for (int k = 0; k < LP_TAPS; ++k) tap[k] = reinterpret_cast<float*>(ws + p.tap[k]);
    float* const by_conv[VG_CONVS] = {s0, tap[0], s0, tap[1], s0, s1, tap[2], s0, s1, tap[3], s0, s1, tap[4]};
    std::copy(by_conv, by_conv + VG_CONVS, t);
}

// One data-gradient launch over tower a's N images of an Ho x Wo map; the plane size follows the map's width, as in vg_conv_launch.
template <int CG, int CX, bool UNPOOL, bool MASK, bool CAN_BE_WIDE>
void vg_dgrad_launch(const float* g, const float* pool, const float* act, float* out, const float* w, int N, int Ho, int Wo, hipStream_t s) {
    const VgDgradArgs a{g, pool, act, out, w, (long long)N * Ho * Wo, Ho, Wo};
    const dim3 grid((unsigned)((a.total + LP_NT - 1) / LP_NT), CX / LP_MT);
    if (vg_stage_bound(Ho, Wo) <= LP_XPOS) {
        hipLaunchKernelGGL((k_vgg_dgrad<CG, CX, UNPOOL, MASK, LP_XPOS>), grid, dim3(D_THREADS), 0, s, a);
    } else if constexpr (CAN_BE_WIDE) {
        hipLaunchKernelGGL((k_vgg_dgrad<CG, CX, UNPOOL, MASK, VG_XPOS_WIDE>), grid, dim3(D_THREADS), 0, s, a);
    }
}
}  // namespace

extern "C" {

int cid_vgg_create(cid_vgg_t* out) {
    if (!out) return CID_ERR_INVALID;
    *out = nullptr;
    cid_vgg_s* h = new (std::nothrow) cid_vgg_s();
    if (!h) return CID_ERR_INVALID;
    h->init("cid_vgg", vg_key_table());
    *out = h;
    return CID_OK;
}

void cid_vgg_destroy(cid_vgg_t h) { delete h; }

const char* cid_vgg_last_error(cid_vgg_t h) { return h ? h->err.c_str() : "null handle"; }

const char* cid_vgg_param_key(cid_vgg_t h, int i) { return h ? h->key(i) : nullptr; }

int cid_vgg_set_weight(cid_vgg_t h, const char* key, const void* data, const int64_t* shape, int ndim) {
    return h ? h->set(key, data, shape, ndim) : CID_ERR_INVALID;
}

int cid_vgg_missing_weights(cid_vgg_t h, int* count) {
    if (!h || !count) return CID_ERR_INVALID;
    *count = h->missing();
    return CID_OK;
}

size_t cid_vgg_packed_weights_bytes(cid_vgg_t h) { return h ? vg_blob_floats() * sizeof(float) : 0; }

int cid_vgg_upload_weights(cid_vgg_t h, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    if (!device_blob) return h->fail(CID_ERR_INVALID, "cid_vgg_upload_weights: null device pointer");
    // all 33 tensors, or exactly the 14 of slice1 ... slice3 (key table entries 2 ... 15); this state check comes ahead of the
    // blob's alignment check, which the shared upload makes
    int set = 0, content = 0;
    for (size_t i = 0; i < h->have.size(); ++i) {
        set += h->have[i] != 0;
        content += h->have[i] && i >= 2 && i < 2 + 2 * (size_t)kVgContentConvs;
    }
    const bool full = set == CID_VGG_NUM_WEIGHTS;
    if (!full && !(set == 2 * kVgContentConvs && content == set))
        return h->fail(CID_ERR_STATE, "cid_vgg_upload_weights: needs all " + std::to_string(CID_VGG_NUM_WEIGHTS) +
                                          " tensors or exactly the 14 of slice1 ... slice3; " + std::to_string(set) + " set, first missing " +
                                          h->keys[h->first_missing()].name);
    const int rc = h->upload(device_blob, stream, vg_blob_floats(), [h, full](float* b) { vg_pack(h, b, full); }, false);
    if (rc == CID_OK) {
        h->full = full;
        h->dev_bwd = nullptr;   // packed from the previous weights
    }
    return rc;
}

int cid_vgg_workspace_bytes(int what, int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    VgPlan p;
    const int rc = vg_plan(what, N, H, W, p);
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

int cid_vgg_stage_view(int what, const char* stage, int N, int H, int W, size_t* offset_bytes, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    VgPlan p;
    const int rc = vg_plan(what, N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    if (s.size() != 5 || s.compare(0, 4, "relu") != 0 || s[4] < '1' || s[4] > (what == CID_VGG_LPIPS ? '5' : '3')) return CID_ERR_KEY;
    const int k = s[4] - '1';
    *offset_bytes = p.tap[k];
    *C = VgTaps::channels(k);
    *Hs = p.Hs[k];
    *Ws = p.Ws[k];
    *channel_block = 8;
    return CID_OK;
}

int cid_vgg_lpips(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
                  double* layers, void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    VgPlan p;
    const int rc = vg_check(h, "cid_vgg_lpips", CID_VGG_LPIPS, a, fmt_a, b, fmt_b, N, H, W, flags, out, layers, workspace, workspace_bytes, p);
    if (rc != CID_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, std::string("cid_vgg_lpips: ") + what + ": " + hipGetErrorString(hipGetLastError())); };
    char* ws = static_cast<char*>(workspace);
    float* t[VG_CONVS];
    vg_plain_tensors(p, ws, t);
    if (const char* failed = vg_features(h, t, p.Hs, p.Ws, a, fmt_a, b, fmt_b, N, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0, true, VG_CONVS, s))
        return herr(failed);
    LpDistArgs da;
    for (int k = 0; k < LP_TAPS; ++k) {
        da.tap[k] = reinterpret_cast<const float*>(ws + p.tap[k]);
        da.P[k] = p.Hs[k] * p.Ws[k];
    }
    da.lin = h->dev_blob + vg_conv_off(VG_CONVS);
    da.out = out;
    da.layers = layers;
    da.N = N;
    hipLaunchKernelGGL(k_lpips_dist<VgTaps>, dim3((unsigned)N), dim3(D_THREADS), 0, s, da);
    if (hipPeekAtLastError() != hipSuccess) return herr("distance");
    return CID_OK;
}

int cid_vgg_content_loss(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags, double* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    VgPlan p;
    const int rc = vg_check(h, "cid_vgg_content_loss", CID_VGG_CONTENT, a, fmt_a, b, fmt_b, N, H, W, flags, out, nullptr, workspace, workspace_bytes, p);
    if (rc != CID_OK) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, std::string("cid_vgg_content_loss: ") + what + ": " + hipGetErrorString(hipGetLastError())); };
    char* ws = static_cast<char*>(workspace);
    float* t[VG_CONVS];
    vg_plain_tensors(p, ws, t);
    if (const char* failed = vg_features(h, t, p.Hs, p.Ws, a, fmt_a, b, fmt_b, N, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0, false, kVgContentConvs, s))
        return herr(failed);
    const VgContentArgs ca{reinterpret_cast<const float*>(ws + p.tap[2]), out, (long long)256 * p.Hs[2] * p.Ws[2], N};
    hipLaunchKernelGGL(k_vgg_content, dim3((unsigned)N), dim3(D_THREADS), 0, s, ca);
    if (hipPeekAtLastError() != hipSuccess) return herr("loss");
    return CID_OK;
}

int cid_vgg_saved_bytes(int N, int H, int W, size_t* bytes) {
    if (!bytes) return CID_ERR_INVALID;
    VgSavedPlan p;
    const int rc = vg_saved_plan(N, H, W, p);
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

int cid_vgg_saved_view(const char* stage, int N, int H, int W, size_t* offset_bytes, int* images, int* C, int* Hs, int* Ws, int* channel_block) {
    if (!stage || !offset_bytes || !images || !C || !Hs || !Ws || !channel_block) return CID_ERR_INVALID;
    VgSavedPlan p;
    const int rc = vg_saved_plan(N, H, W, p);
    if (rc != CID_OK) return rc;
    const std::string s(stage);
    for (int i = 0; i < kVgSaved; ++i) {
        const bool act = s == kVgActName[i];
        if (!act && s != kVgGradName[i]) continue;
        const int k = act ? kVgActLevel[i] : kVgGradLevel[i];
        *offset_bytes = act ? p.act[i] : p.grad[i];
        *images = act ? 2 * N : N;
        *C = act ? VgTaps::channels(k) : kVgGradC[i];
        *Hs = p.Hs[k];
        *Ws = p.Ws[k];
        *channel_block = 8;
        return CID_OK;
    }
    return CID_ERR_KEY;
}

int cid_vgg_content_loss_saved(cid_vgg_t h, const void* a, int fmt_a, const void* b, int fmt_b, int N, int H, int W, unsigned flags,
                               double* out, void* saved, size_t saved_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    VgPlan fp;
    const int rc = vg_check(h, "cid_vgg_content_loss_saved", CID_VGG_CONTENT, a, fmt_a, b, fmt_b, N, H, W, flags, out, nullptr, saved, saved_bytes, fp, true);
    if (rc != CID_OK) return rc;
    VgSavedPlan p;
    vg_saved_plan(N, H, W, p);
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, std::string("cid_vgg_content_loss_saved: ") + what + ": " + hipGetErrorString(hipGetLastError())); };
    char* sv = static_cast<char*>(saved);
    float* t[kVgSaved];
    for (int i = 0; i < kVgSaved; ++i) t[i] = reinterpret_cast<float*>(sv + p.act[i]);
    if (const char* failed = vg_features(h, t, p.Hs, p.Ws, a, fmt_a, b, fmt_b, N, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0, false, kVgContentConvs, s))
        return herr(failed);
    const VgContentArgs ca{t[6], out, (long long)256 * p.Hs[2] * p.Ws[2], N};
    hipLaunchKernelGGL(k_vgg_content, dim3((unsigned)N), dim3(D_THREADS), 0, s, ca);
    if (hipPeekAtLastError() != hipSuccess) return herr("loss");
    return CID_OK;
}

size_t cid_vgg_backward_weights_bytes(cid_vgg_t h) { return h ? vg_bwd_floats() * sizeof(float) : 0; }

int cid_vgg_upload_backward_weights(cid_vgg_t h, void* device_blob, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const std::string fn = "cid_vgg_upload_backward_weights: ";
    if (!device_blob) return h->fail(CID_ERR_INVALID, fn + "null device pointer");
    for (int i = 2; i < 2 + 2 * kVgContentConvs; ++i)
        if (!h->have[i]) return h->fail(CID_ERR_STATE, fn + h->keys[i].name + " not set");
    if ((uintptr_t)device_blob & 255) return h->fail(CID_ERR_WORKSPACE, fn + "blob must be 256-byte aligned");
    h->bwd_staging.assign(vg_bwd_floats(), 0.f);
    vg_pack_backward(h, h->bwd_staging.data());
    hipStream_t s = static_cast<hipStream_t>(stream);
    hipError_t e = hipMemcpyAsync(device_blob, h->bwd_staging.data(), h->bwd_staging.size() * sizeof(float), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);   // the staging copy is pageable
    if (e != hipSuccess) return h->fail(CID_ERR_HIP, fn + hipGetErrorString(e));
    h->dev_bwd = static_cast<const float*>(device_blob);
    return CID_OK;
}

int cid_vgg_content_backward(cid_vgg_t h, const double* grad_out, float* grad_a, int N, int H, int W, unsigned flags, void* saved,
                             size_t saved_bytes, void* stream) {
    if (!h) return CID_ERR_INVALID;
    const std::string f = "cid_vgg_content_backward";
    if (!grad_out || !grad_a || !saved) return h->fail(CID_ERR_INVALID, f + ": null pointer");
    if (((uintptr_t)grad_out & 7) || ((uintptr_t)grad_a & 3)) return h->fail(CID_ERR_INVALID, f + ": misaligned operand");
    if (flags & ~(unsigned)CID_LPIPS_UNIT_VIEW) return h->fail(CID_ERR_INVALID, f + ": unknown flags");
    VgSavedPlan p;
    if (vg_saved_plan(N, H, W, p) != CID_OK)
        return h->fail(CID_ERR_SHAPE, f + ": shape not accepted (1 <= N <= 2^20, 4 <= H, W <= " + std::to_string(VG_MAX_SIDE) + ", 2 N H W < 2^37)");
    if (saved_bytes < p.total || ((uintptr_t)saved & 255))
        return h->fail(CID_ERR_WORKSPACE, f + ": saved arena smaller than cid_vgg_saved_bytes() or not 256-byte aligned");
    if (!h->dev_blob) return h->fail(CID_ERR_STATE, f + ": weights not uploaded");
    if (!h->dev_bwd) return h->fail(CID_ERR_STATE, f + ": backward weights not uploaded (cid_vgg_upload_backward_weights)");
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto herr = [&](const char* what) { return h->fail(CID_ERR_HIP, f + ": " + what + ": " + hipGetErrorString(hipGetLastError())); };
    const auto bad = [] { return hipPeekAtLastError() != hipSuccess; };
    char* sv = static_cast<char*>(saved);
    const float* act[kVgSaved];
    float* g[kVgSaved];
    for (int i = 0; i < kVgSaved; ++i) {
        act[i] = reinterpret_cast<const float*>(sv + p.act[i]);
        g[i] = reinterpret_cast<float*>(sv + p.grad[i]);
    }
    const float* bw = h->dev_bwd;
    const int H1 = p.Hs[0], W1 = p.Ws[0], H2 = p.Hs[1], W2 = p.Ws[1], H3 = p.Hs[2], W3 = p.Ws[2];
    {
        VgSeedArgs sa{act[6], grad_out, g[0], (long long)256 * H3 * W3, 0, N};
        sa.total = sa.count * N;
        hipLaunchKernelGGL(k_vgg_seed, dim3((unsigned)((sa.total / 4 + D_THREADS - 1) / D_THREADS)), dim3(D_THREADS), 0, s, sa);
        if (bad()) return herr("grad3_3");
    }
    vg_dgrad_launch<256, 256, false, true, false>(g[0], nullptr, act[5], g[1], bw + vg_bwd_off(6), N, H3, W3, s);
    if (bad()) return herr("grad3_2");
    vg_dgrad_launch<256, 256, false, true, false>(g[1], nullptr, act[4], g[2], bw + vg_bwd_off(5), N, H3, W3, s);
    if (bad()) return herr("grad3_1");
    vg_dgrad_launch<256, 128, false, false, false>(g[2], nullptr, nullptr, g[3], bw + vg_bwd_off(4), N, H3, W3, s);
    if (bad()) return herr("gradpool2");
    vg_dgrad_launch<128, 128, true, true, false>(g[3], act[3], act[2], g[4], bw + vg_bwd_off(3), N, H2, W2, s);
    if (bad()) return herr("grad2_1");
    vg_dgrad_launch<128, 64, false, false, false>(g[4], nullptr, nullptr, g[5], bw + vg_bwd_off(2), N, H2, W2, s);
    if (bad()) return herr("gradpool1");
    vg_dgrad_launch<64, 64, true, true, true>(g[5], act[1], act[0], g[6], bw + vg_bwd_off(1), N, H1, W1, s);
    if (bad()) return herr("grad1_1");
    {
        const VgHeadBwdArgs ha{g[6], grad_a, bw, (long long)N * H * W, H, W, (flags & CID_LPIPS_UNIT_VIEW) != 0};
        hipLaunchKernelGGL(k_vgg_head_bwd, dim3((unsigned)((ha.total + VG_HEAD_PIX - 1) / VG_HEAD_PIX)), dim3(VG_HEAD_PIX), 0, s, ha);
        if (bad()) return herr("grad_a");
    }
    return CID_OK;
}

}  // extern "C"
