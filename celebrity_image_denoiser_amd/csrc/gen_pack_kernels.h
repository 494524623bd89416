// gen_pack_kernels.h — the generator's packed weights blob built from the 24 parameter tensors: THE definition of the blob's layouts.
//
// One piece of source compiled twice.  On the device k_gen_pack writes every segment of BlobLayout (cid_api.hip), the four LDS slot
// tables and the alignment gaps (zeros); a training loop calls it after every optimizer step in place of 24 device-to-host copies, a
// host repack and one 58.7 MB upload.  On the host cid_set_weight runs gen_pack_produce over the work items of the segments that one
// tensor feeds, and cid_handle_s's constructor over those of the tables.  Each family's layout (index order, which MFMA operand a lane
// holds) is described where its formula stands below; the kernels' comments point here.
//
// Gather form: a lane owns 16 bytes of the blob (a "quad": four fp32 words or eight halfs), a wave a "tile" of 64 consecutive quads
// (1 KiB) of ONE segment: tiles are counted per segment (the last tile of a segment may be partly masked), so that the segment, found by
// binary search in a table that lies in the kernel arguments, and every index that a tile's quads share are wave-uniform: they live
// in scalar registers and the divisions of the decode run on the scalar unit.  A lane inverts its segment's index formula into
// (co, ci, kh, kw), reads the parameter(s) with 4-byte loads and stores one uint4 per tile.  Every segment starts on a 256-byte
// boundary and its quads run up to the next one's start, so every byte is written exactly once by construction; there are no
// atomics and nothing is read from the blob.  Next to each inverse stands the forward formula (the index of element (co, ci, tap) in
// the segment), which is what the consuming kernel relies on.  tests/golden/gen_pack_digests.json, recorded from the separate scatter
// pack that the host had before, pins the layout; the byte-identity test (tests/test_generator_pack_device.py) holds the device's
// arithmetic and stores against the host's run of the same source.
//
// The layouts are transposes of the reference tensors, so a wave's 4-byte reads are scattered (one cache line per lane and load) and
// the kernel is paced by them, not by its stores.  Where several tiles need the same parameters in the same lanes, one wave therefore
// takes the whole group as one work item and loads once: the 24 tiles (a, b) of a Winograd F(4x2) position group (four filters per
// lane), the 4 tiles (a) of an F(2x2) one, the hi | lo | hi tiles of a split16 sub-chunk.  Elsewhere a work item is one tile.
//
// Arithmetic that has to come out the same on the host and on the device, bit for bit:
//   * the Winograd filter transforms U = G g G^T run in double (rows first, then columns, the products by 0 and 1 included), rounded
//     once to fp32.  The host is built without FMA; device code is contracted by default, so the transform functions switch
//     contraction off.
//   * half pieces: hi = (_Float16)v, lo = (_Float16)(v - (float)hi), round-to-nearest-even, fp16 subnormals kept.
// Outside the contract (cid.h): fp32-subnormal, |v| > 65504 and non-finite parameter values.
//
// The source reads with 4-byte loads (the ABI promises no more alignment); the compiler merges a lane's consecutive ones into wider
// global loads, which need no more than 4-byte alignment on gfx950.
//
// tools/gen_pack_emu.hip runs all of it on the CPU: every quad is produced exactly once over all work items, and staging tensor by
// tensor in either order gives the whole-blob gather and touches no other tensor's segments.
#pragma once
#include "wino42_kernels.h"

namespace cid {

constexpr int GP_THREADS = 256;
constexpr int GP_MAX_SEGS = 96;

enum GenPackFamily : unsigned char {
    // 4-byte elements
    GP_COPY,         // bias, reference-layout copies: element i = src[i]
    GP_W_HEAD,       // down1.0 for k_conv_head (head_step order)
    GP_W_TAIL,       // upconv1.2 for k_conv_tail: [chunk][group][lane][4], columns 27..31 zero
    GP_W_CONVT_S32,  // up1 for k_convt_s32
    GP_W_GEMM,       // 3x3 layers for k_gemm_conv
    GP_W_GEMM_T,     // up2 for k_gemm_conv, MODE 2
    GP_U,            // Winograd F(2x2,3x3) U
    GP_U42,          // Winograd F(4x2,3x3) U
    GP_TAB,          // LDS slot tables: src = 0, 1 (wino_slot_entry 32x1, 16x2), 2, 3 (wino42_slot_entry<8>, <4>)
    // 2-byte elements
    GP_H_CONV,       // 3x3 layers for k_conv3x3_h16
    GP_H_CONVT,      // up2, up1 for k_convt_t16
    GP_H_TAIL,       // k_conv_tail_h: [s][lane][8]
    GP_H_HEAD,       // k_conv_head_h16: [co & 3][k >> 3][(co >> 2) & 15][8], rows 27..31 zero
    GP_HZ,           // fused last layer's A fragments
    GP_HZS,          // the same as hi | lo pieces
    GP_S_CONV,       // split16 pieces of a 3x3 layer: hi | lo | hi
    GP_S_CONVT,      // split16 pieces of a transposed convolution: hi | lo | hi
};

// One segment of the blob: the nq quads [q0, next segment's q0), work items [t0, t0 + ceil(nq / 64) / gp_group(fam)).  Elements (words or
// halfs) at index >= count are zero: the unused tail of the segment and the alignment gap after it.
struct GenPackSeg {
    unsigned q0, nq, t0, count;
    unsigned short cin, cout;
    unsigned char fam, src;   // src: index into GenPackArgs::p (GP_TAB: which table)
};

struct GenPackArgs {
    const float* p[24];   // cid_param_key order
    uint4* blob;
    unsigned nitems;
    int nseg;
    GenPackSeg seg[GP_MAX_SEGS];
};

// G of F(2,3): {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}}
__host__ __device__ inline double gp_g2(int a, int k) {
    return a == 0 ? (k == 0 ? 1.0 : 0.0) : a == 3 ? (k == 2 ? 1.0 : 0.0) : (a == 2 && k == 1) ? -0.5 : 0.5;
}
// G of F(4,3) at the points 0, 3/4, -3/4, 3/2, -3/2, inf (tests/test_host.py checks them against the kernel's B4^T and A4^T)
__host__ __device__ inline double gp_g4(int b, int k) {
    switch (b * 3 + k) {
        case 0: return 64.0 / 81;
        case 3: case 6: return -128.0 / 243;
        case 4: return -32.0 / 81;
        case 7: return 32.0 / 81;
        case 5: case 8: return -8.0 / 27;
        case 9: case 12: return 32.0 / 243;
        case 10: return 16.0 / 81;
        case 13: return -16.0 / 81;
        case 11: case 14: case 17: return b == 5 ? 1.0 : 8.0 / 27;
        default: return 0.0;   // 1, 2, 15, 16
    }
}
// Tiles per work item (see above).  The grouped families' segments hold whole groups and no padding.
__host__ __device__ constexpr int gp_group(int fam) { return fam == GP_U42 ? 24 : fam == GP_U ? 4 : fam == GP_S_CONV ? 3 : 1; }

// Row a of G2 g for filter g (9 floats) ...
__host__ __device__ inline void gp_wino_row(const float (&g)[9], int a, double (&tmp)[3]) {
#pragma clang fp contract(off)
    for (int q = 0; q < 3; ++q) tmp[q] = gp_g2(a, 0) * g[0 * 3 + q] + gp_g2(a, 1) * g[1 * 3 + q] + gp_g2(a, 2) * g[2 * 3 + q];
}
// ... then position (a, b) of U: column b by F(2,3) (six == false) or by F(4,3).
__host__ __device__ inline float gp_wino_col(const double (&tmp)[3], int b, bool six) {
#pragma clang fp contract(off)
    const double g0 = six ? gp_g4(b, 0) : gp_g2(b, 0), g1 = six ? gp_g4(b, 1) : gp_g2(b, 1), g2 = six ? gp_g4(b, 2) : gp_g2(b, 2);
    const double u = tmp[0] * g0 + tmp[1] * g1 + tmp[2] * g2;
    return (float)u;
}

__host__ __device__ inline unsigned gp_bits(float v) { return __builtin_bit_cast(unsigned, v); }
__host__ __device__ inline unsigned gp_hbits(_Float16 v) { return __builtin_bit_cast(unsigned short, v); }

// Reference-layout index: Conv2d [Cout, Cin, 3, 3] with tap = 3 kh + kw; ConvTranspose2d [Cin, Cout, 2, 2] with tap = 2 kh + kw.
__host__ __device__ inline unsigned gp_ref3(const GenPackSeg& s, int co, int ci, int tap) { return ((unsigned)co * s.cin + ci) * 9 + tap; }
__host__ __device__ inline unsigned gp_reft(const GenPackSeg& s, int co, int ci, int tap) { return ((unsigned)ci * s.cout + co) * 4 + tap; }

// Word k of quad (t, lane) of a 4-byte-element segment: word i = 256 t + 4 lane + k of the segment.  t is wave-uniform.
__host__ __device__ inline unsigned gp_word(const GenPackSeg& s, const float* w, unsigned t, int lane, int k) {
    const unsigned i = 256 * t + 4 * lane + k;
    if (s.fam == GP_TAB) {   // the padded tables fill their segments
        const int e = (int)i;
        return s.src == 0 ? (e < wino_slot_count(32, 1) ? wino_slot_entry(32, 1, e) : 0u)
             : s.src == 1 ? (e < wino_slot_count(16, 2) ? wino_slot_entry(16, 2, e) : 0u)
             : s.src == 2 ? (e < 4 * W42Geom<8>::RW * 64 ? wino42_slot_entry<8>(e) : 0u)
                          : (e < 4 * W42Geom<4>::RW * 64 ? wino42_slot_entry<4>(e) : 0u);
    }
    if (i >= s.count) return 0u;
    switch (s.fam) {
        case GP_COPY: return gp_bits(w[i]);
        case GP_W_HEAD: {   // ((co >> 5) * 14 + step) * 64 + h * 32 + (co & 31), k = ci * 9 + tap on lane half h of MFMA step `step`: the head's K order
                            // (conv_kernels.h head_step); a half with no element (-1) holds a zero weight
            const int j = i & 31, h = (i >> 5) & 1, r = i >> 6, step = r % 14, co = 32 * (r / 14) + j;
            const HeadStep hs = head_step(step);
            const int kk = h ? hs.k1 : hs.k0;
            return kk < 0 ? 0u : gp_bits(w[co * 27 + kk]);
        }
        case GP_W_TAIL: {   // ((ck * 4 + g) * 64 + h * 32 + col) * 4 + e, ci = 32 ck + 8 g + 4 h + e, col = 3 tap + co: B[k = ci][col] of the tail's
                            // 64 x 32 product, columns 27..31 zero
            const int e = i & 3, col = (i >> 2) & 31, h = (i >> 7) & 1, g = (i >> 8) & 3, ck = i >> 10;
            return col >= 27 ? 0u : gp_bits(w[gp_ref3(s, col % 3, 32 * ck + 8 * g + 4 * h + e, col / 3)]);
        }
        case GP_W_CONVT_S32: {   // ((((tap * (cin / 16) + g) * 4 + j) * 4 + mt) * 64) + kga * 16 + row, ci = 16 g + 4 kga + j, co = 16 mt + row:
                                 // lane 16 kga + row holds A[row][k = kga] of v_mfma_f32_16x16x4_f32 for k-step j of group g
            const int row = 4 * (lane & 3) + k, kga = (lane >> 2) & 3, mt = lane >> 4, j = t & 3, r = t >> 2, ng = s.cin / 16, g = r % ng, tap = r / ng;
            return gp_bits(w[gp_reft(s, 16 * mt + row, 16 * g + 4 * kga + j, tap)]);
        }
        case GP_W_GEMM:
        case GP_W_GEMM_T: {   // ((((nb * nchunk + ck) * taps + tap) * 4 + g) * 2 + ns) * 256 + (h * 32 + j) * 4 + e, ci = 32 ck + 8 g + 4 h + e,
                              // n' = 64 nb + 32 ns + j: lane (h, j) of v_mfma_f32_32x32x2_f32 holds B[k = h][col = j]; e walks the 4 MFMAs of group g
            const bool tr = s.fam == GP_W_GEMM_T;
            const int e = k, j = lane & 31, h = lane >> 5, ns = t & 1, g = (t >> 1) & 3, r = t >> 3;
            const int taps = tr ? 1 : 9, nchunk = s.cin / 32, tap = r % taps, r2 = r / taps, ck = r2 % nchunk, nb = r2 / nchunk;
            const int np = 64 * nb + 32 * ns + j, ci = 32 * ck + 8 * g + 4 * h + e;   // n' = co, or tap * COUT + co for the transposed layer
            return gp_bits(tr ? w[gp_reft(s, np % s.cout, ci, np / s.cout)] : w[gp_ref3(s, np, ci, tap)]);
        }
        default: return 0u;
    }
}

// Half e of quad (t, lane) of a 2-byte-element segment: half i = 512 t + 8 lane + e of the segment.
__host__ __device__ inline unsigned gp_half(const GenPackSeg& s, const float* w, unsigned t, int lane, int e) {
    const unsigned i = 512 * t + 8 * lane + e;
    if (i >= s.count) return 0u;
    const int l16 = lane & 15, l4 = lane >> 4;   // lane = 16 l4 + l16 of every fragment layout below
    float v;
    bool lo = false;
    switch (s.fam) {
        // k_conv3x3_h16: lane (col c, kg) of v_mfma_f32_16x16x32_f16 holds B[k = 8 kg .. 8 kg + 7][col] with ci = 32 ck + 8 kg + e; column c of
        // channel group cg is output channel 64 nb + 4 c + cg, so a lane's four accumulator tiles are four consecutive channels (the
        // kernel stores them as 8 bytes); one (chunk, kw) is a 12 KiB LDS-DMA unit.  split16 (k_conv3x3_h16<F32IO>): sub-chunk j = 0..2
        // is tap column kw = j of hi_w (met by hi_x), 3..5 of lo_w (met by hi_x), 6..8 of hi_w again (met by lo_x); hi_w = half(w),
        // lo_w = half(w - hi_w)
        case GP_H_CONV:     // ((((((nb * nchunk + ck) * 3 + kw) * 3 + kh) * 4 + cg) * 64) + kg * 16 + c) * 8 + e
        case GP_S_CONV: {   // ((((((nb * nchunk + ck) * 9 + j) * 3 + kh) * 4 + cg) * 64) + kg * 16 + c) * 8 + e, j = 3 piece + kw
            const int cg = t & 3, nj = s.fam == GP_S_CONV ? 9 : 3, nchunk = s.cin / 32;
            int r = t >> 2;
            const int kh = r % 3; r /= 3;
            const int j = r % nj; r /= nj;
            const int ck = r % nchunk, nb = r / nchunk, kw = j % 3;
            lo = j / 3 == 1;
            v = w[gp_ref3(s, 64 * nb + 4 * l16 + cg, 32 * ck + 8 * l4 + e, 3 * kh + kw)];
            break;
        }
        // k_convt_t16: the A operand of v_mfma_f32_16x16x32_f16, A[row][k = 8 kga + e] with ci = 32 ks + 8 kga + e; row `row` of M tile mt is
        // channel 64 cb + 32 (mt >> 1) + 8 (row >> 2) + 4 (mt & 1) + (row & 3), so a lane's two M tiles of a pair are eight consecutive channels
        case GP_H_CONVT: {   // (((((tap * CB + cb) * KS + ks) * 4 + mt) * 64) + kga * 16 + row) * 8 + e
            const int mt = t & 3, KS = s.cin / 32, CB = s.cout / 64;
            int r = t >> 2;
            const int ks = r % KS; r /= KS;
            const int cb = r % CB, tap = r / CB;
            const int c = ((mt >> 1) << 5) | ((l16 >> 2) << 3) | ((mt & 1) << 2) | (l16 & 3);
            v = w[gp_reft(s, 64 * cb + c, 32 * ks + 8 * l4 + e, tap)];
            break;
        }
        case GP_S_CONVT: {   // ((((((blk * nchunk + ck) * 3 + p) * 4 + cg) * 64) + kg * 16 + c) * 8 + e, blk = tap * (cout / 64) + co / 64; piece p = 0 hi_w,
                             // 1 lo_w, 2 hi_w again (met by lo_x), lanes as GP_H_CONV (k_conv3x3_h16<..., 2, ., ., F32IO, PAIR>)
            const int cg = t & 3, nchunk = s.cin / 32, cbs = s.cout / 64;
            int r = t >> 2;
            const int p = r % 3; r /= 3;
            const int ck = r % nchunk, blk = r / nchunk;
            lo = p == 1;
            v = w[gp_reft(s, 64 * (blk % cbs) + 4 * l16 + cg, 32 * ck + 8 * l4 + e, blk / cbs)];
            break;
        }
        case GP_H_TAIL: {   // (s * 64 + hh * 32 + col) * 8 + e, ci = 16 s + 8 hh + e, col = 3 tap + co: k_conv_tail_h's [k-step s][lane = 32 hh + col][e]
            const int col = lane & 31, hh = lane >> 5, st = t;
            if (col >= 27) return 0u;
            v = w[gp_ref3(s, col % 3, 16 * st + 8 * hh + e, col / 3)];
            break;
        }
        case GP_H_HEAD: {   // ((co & 3) * 64 + (k >> 3) * 16 + ((co >> 2) & 15)) * 8 + (k & 7), k = 3 tap + c: k_conv_head_h16's B[k][co], rows 27..31
                            // zero; lane (col = (co / 4) % 16, kg) of group co % 4 holds k = 8 kg .. 8 kg + 7
            const int k = 8 * l4 + e, co = 4 * l16 + (int)t;
            if (k >= 27) return 0u;
            v = w[gp_ref3(s, co, k % 3, k / 3)];
            break;
        }
        case GP_HZ:
        case GP_HZS: {   // [piece][row tile rt][k-step ks][lane = 16 kga + row][e], row 16 rt + row = 3 tap + co, ci = 32 ks + 8 kga + e: the A operand of
                         // z^T = W2' . X^T on v_mfma_f32_16x16x32_f16 (h16_zout_epilogue), 27 rows, rows 27..31 zero; GP_HZS: hi | lo pieces
            const int ks = t & 1, rt = (t >> 1) & 1, row = 16 * rt + l16;
            lo = s.fam == GP_HZS && (t >> 2) == 1;
            if (row >= 27) return 0u;
            v = w[gp_ref3(s, row % 3, 32 * ks + 8 * l4 + e, row / 3)];
            break;
        }
        default: return 0u;
    }
    const _Float16 hi = (_Float16)v;
    return gp_hbits(lo ? (_Float16)(v - (float)hi) : hi);
}

// Work items of the grouped families: emit(q, words) stores the quad at blob offset 16 q.
// GP_U: Winograd F(2x2,3x3) filter transform U = G g G^T, 16 values per (co, ci), laid out for k_wino64_conv:
// [co / 64][ci / 16][(ci / 8) % 2][a][(co / 32) % 2][e][lane = 32 h + j][b], ci = 16 ck + 8 g2 + 4 h + e, co = 64 nb + 32 nt + j (one quad per lane =
// the four positions b of k-step e, so a quad's registers free up after 4 MFMAs); item t = the same without a
template <class Emit>
__host__ __device__ inline void gp_item_u(const GenPackSeg& s, const float* w, unsigned t, int lane, Emit&& emit) {
    const int j = lane & 31, h = lane >> 5, e = t & 3, nt = (t >> 2) & 1, g2 = (t >> 3) & 1;
    const int r = t >> 4, nchunk = s.cin / 16, ck = r % nchunk, nb = r / nchunk;
    const float* src = w + gp_ref3(s, 64 * nb + 32 * nt + j, 16 * ck + 8 * g2 + 4 * h + e, 0);
    float g[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) g[k] = src[k];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double tmp[3];
        gp_wino_row(g, a, tmp);
        unsigned out[4];
#pragma unroll
        for (int b = 0; b < 4; ++b) out[b] = gp_bits(gp_wino_col(tmp, b, false));
        const unsigned tile = ((((unsigned)r * 2 + g2) * 4 + a) * 2 + nt) * 4 + e;
        emit(s.q0 + 64 * tile + lane, out);
    }
}
// GP_U42: Winograd F(4x2,3x3) filter transform U = G2 g G4^T, rows by F(2,3), columns by F(4,3): 24 values per (co, ci), laid out for k_wino42_conv:
// [co / 64][unit][a][q = 6 e2 + b][lane = 16 gg + j][cg], ci = 16 (unit / 2) + 4 gg + 2 ((unit % 2) ^ (gg & 1)) + e2, co = 64 nb + 4 j + cg (one quad per
// lane = the four channel groups of position (a, b) at k-step e2: one V value, four MFMAs; column j of channel group cg = channel 4 j + cg: see
// the kernel's epilogue).  Lane group gg reads the 8-byte half (ci >> 1) & 1 of its LDS quad for unit % 2 = half ^ (gg & 1): odd lane groups
// take the halves in the other order, which makes the kernel's ds_read_b64 conflict-free (wino42_kernels.h, xbase / ybase).
// item t = (nb * nunit + unit) * 2 + e2
template <class Emit>
__host__ __device__ inline void gp_item_u42(const GenPackSeg& s, const float* w, unsigned t, int lane, Emit&& emit) {
    const int j = lane & 15, gg = lane >> 4, e2 = t & 1, r = t >> 1, nunit = s.cin / 8, unit = r % nunit, nb = r / nunit;
    const int ci = 16 * (unit >> 1) + 4 * gg + 2 * ((unit & 1) ^ (gg & 1)) + e2;
    float g[4][9];
#pragma unroll
    for (int cg = 0; cg < 4; ++cg) {
        const float* src = w + gp_ref3(s, 64 * nb + 4 * j + cg, ci, 0);
#pragma unroll
        for (int k = 0; k < 9; ++k) g[cg][k] = src[k];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        double tmp[4][3];
#pragma unroll
        for (int cg = 0; cg < 4; ++cg) gp_wino_row(g[cg], a, tmp[cg]);
#pragma unroll
        for (int b = 0; b < 6; ++b) {
            unsigned out[4];
#pragma unroll
            for (int cg = 0; cg < 4; ++cg) out[cg] = gp_bits(gp_wino_col(tmp[cg], b, true));
            const unsigned tile = ((unsigned)r * 4 + a) * 12 + 6 * e2 + b;
            emit(s.q0 + 64 * tile + lane, out);
        }
    }
}
// GP_S_CONV: ((((((nb * nchunk + ck) * 9 + j) * 3 + kh) * 4 + cg) * 64) + kg * 16 + c) * 8 + e, j = 3 piece + kw, pieces hi | lo | hi;
// item t = (((nb * nchunk + ck) * 3 + kw) * 3 + kh) * 4 + cg
template <class Emit>
__host__ __device__ inline void gp_item_s_conv(const GenPackSeg& s, const float* w, unsigned t, int lane, Emit&& emit) {
    const int l16 = lane & 15, l4 = lane >> 4, cg = t & 3, nchunk = s.cin / 32;
    int r = t >> 2;
    const int kh = r % 3; r /= 3;
    const int kw = r % 3; r /= 3;
    const int ck = r % nchunk, nb = r / nchunk;
    unsigned hi[4], lo[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        unsigned ph[2], pl[2];
#pragma unroll
        for (int x = 0; x < 2; ++x) {
            const float v = w[gp_ref3(s, 64 * nb + 4 * l16 + cg, 32 * ck + 8 * l4 + 2 * k + x, 3 * kh + kw)];
            const _Float16 vh = (_Float16)v;
            ph[x] = gp_hbits(vh);
            pl[x] = gp_hbits((_Float16)(v - (float)vh));
        }
        hi[k] = ph[0] | ph[1] << 16;
        lo[k] = pl[0] | pl[1] << 16;
    }
#pragma unroll
    for (int p = 0; p < 3; ++p) {
        const unsigned tile = ((((unsigned)r * 9 + 3 * p + kw) * 3 + kh) * 4) + cg;
        emit(s.q0 + 64 * tile + lane, p == 1 ? lo : hi);
    }
}

// The last segment that starts at or before work item `item`.
__host__ __device__ inline int gen_pack_find(const GenPackArgs& a, unsigned item) {
    int lo = 0, hi = a.nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.seg[mid].t0 <= item) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// Work item t (wave-uniform) of segment s as seen by lane `lane`: emit(q, words) for each of the lane's quads.  w = the segment's
// parameter tensor (GP_TAB reads none).
template <class Emit>
__host__ __device__ inline void gen_pack_produce(const GenPackSeg& s, const float* w, unsigned t, int lane, Emit&& emit) {
    if (s.fam == GP_U42) return gp_item_u42(s, w, t, lane, emit);
    if (s.fam == GP_U) return gp_item_u(s, w, t, lane, emit);
    if (s.fam == GP_S_CONV) return gp_item_s_conv(s, w, t, lane, emit);
    const unsigned r = 64 * t + lane;   // one tile
    if (r >= s.nq) return;
    unsigned out[4];
    if (s.fam < GP_H_CONV) {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = gp_word(s, w, t, lane, k);
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) out[k] = gp_half(s, w, t, lane, 2 * k) | gp_half(s, w, t, lane, 2 * k + 1) << 16;
    }
    emit(s.q0 + r, out);
}

// Work item `item` of the whole blob: search, then produce.
template <class Emit>
__host__ __device__ inline void gen_pack_item(const GenPackArgs& a, unsigned item, int lane, Emit&& emit) {
    const GenPackSeg s = a.seg[gen_pack_find(a, item)];
    const float* w = s.fam == GP_TAB ? nullptr : a.p[s.src];
    const unsigned t = item - s.t0;
    gen_pack_produce(s, w, t, lane, emit);
}

__global__ void __launch_bounds__(GP_THREADS) k_gen_pack(const GenPackArgs a) {
    // one work item per wave; the wave's index through readfirstlane so that the compiler keeps what follows from it in scalar registers
    const unsigned item = blockIdx.x * (GP_THREADS / 64) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (item >= a.nitems) return;
    uint4* blob = a.blob;
    gen_pack_item(a, item, threadIdx.x & 63, [blob](unsigned q, const unsigned (&v)[4]) { blob[q] = make_uint4(v[0], v[1], v[2], v[3]); });
}

}  // namespace cid
