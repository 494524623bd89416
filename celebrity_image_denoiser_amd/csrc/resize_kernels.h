// resize_kernels.h — gfx950 device kernel of the bicubic resize (cid_resize, include/cid.h): PIL's Image.resize(size, BICUBIC) on
// uint8 NHWC batches, the first step of every reference entry point (noise_generation.py:61, denoisegan_eval.py,
// denoise_eavl_iter.py:89, training.py:303-304), bit for bit.  The arithmetic is integer: 22-bit fixed-point coefficients built on
// the host (resize_tables in api/resize.h, restated as synth.resize_tables_np), a horizontal pass into a uint8 intermediate, a
// vertical pass over that intermediate, each out = clamp((2^21 + sum in * k) >> 22, 0, 255) in int32.
//
// k_resize<MODE>: ONE launch per call; a workgroup of RESIZE_THREADS owns a tile of TR x TC output pixels of one image (the plan
// picks TR and TC, powers of two, so that the LDS below stays within RESIZE_LDS_BUDGET).
//   RM_BOTH   the tile's TR output rows need the source rows [r0, r1) = [vb[first].min, vb[last].min + vb[last].n) and its TC output
//             columns the source columns [c0, c1) likewise.  In chunks of SR rows, those source rows' bytes [c0*3, c1*3) are staged
//             into LDS (stage_rows: 16-byte loads where the 16-byte unit lies inside the span, byte by byte in the head and the tail
//             unit, as k_adam_step treats its head and tail; no byte outside the span is read), the horizontal pass runs from the stage
//             into the BAND, (r1 - r0) x TC x 3 bytes of LDS: the uint8 intermediate never goes to memory.  Then the vertical pass
//             runs out of the band and stores the tile.
//   RM_HONLY  (Hs == Hd) the same staging and horizontal pass over the tile's own TR rows, stored directly.
//   RM_VONLY  (Ws == Wd) the tile's source rows x its own columns are staged straight into the band, then the vertical pass.
//   RM_COPY   (neither) one pixel per lane, read and stored.
// Loop bounds are uniform per tile (the tile's largest n, from the plan's per-tile table); a lane's own (min, n) mask the tail by a
// predicate.  The multiply is uint8 x a coefficient below 2^23 in magnitude (checked by the plan): v_mad_i32_i24.  No atomics;
// every output element is written once by one lane; LDS is written before it is read (barriers between the phases).
// Output: uint8 NHWC, or fp32 NCHW as (u/255.0f - 0.5f)/0.5f with true divisions — the head kernel's IN_U8 expression
// (conv_kernels.h), so that the float result fed to cid_forward gives the bits of the uint8 result fed to the uint8 forward.
// Offsets into the batch are 64-bit.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cid {

constexpr int RESIZE_THREADS = 256;
// LDS per workgroup (band + stage).  160 KiB per CU / 32 KiB = 5 workgroups = 20 waves per CU by LDS, so that one workgroup's
// staging loads overlap the others' passes; the kernel's registers allow more, LDS is the limit.
constexpr int RESIZE_LDS_BUDGET = 32 * 1024;
constexpr int RESIZE_MAX_GRID_Y = 65535;   // images per grid row; larger batches loop in the kernel

enum ResizeMode { RM_COPY = 0, RM_HONLY = 1, RM_VONLY = 2, RM_BOTH = 3 };

struct ResizeAxis {
    const int* bounds;   // [out][2] = (min, n)
    const int* coeffs;   // horizontal: TRANSPOSED [ksize][out] (lanes of consecutive columns read consecutive words);
                         // vertical: [out][ksize] (a row's coefficients are uniform over its lanes)
    const int* tile_n;   // [tiles of this axis]: the largest n of the tile's outputs
    int ksize;
};

struct ResizeArgs {
    const uint8_t* src;  // [N][Hs][Ws][3]
    void* dst;           // uint8 [N][Hd][Wd][3] or fp32 [N][3][Hd][Wd]
    int N, Hs, Ws, Hd, Wd;
    int f32;             // 0: CID_FMT_U8_NHWC, 1: CID_FMT_F32_NCHW
    int TR, TC;          // tile, powers of two, TC <= RESIZE_THREADS
    int tiles_x;
    int band_pitch;      // bytes per band row
    int stage_pitch;     // bytes per stage row, a multiple of 16 >= 15 + 3 * (widest source span of a tile)
    int SR;              // stage rows per chunk
    int band_bytes;      // offset of the stage in LDS (a multiple of 16)
    ResizeAxis h, v;
};

__device__ __forceinline__ int resize_clip8(int acc) {
    const int v = acc >> 22;
    return v < 0 ? 0 : (v > 255 ? 255 : v);
}

// Copies bytes [0, nbytes) of `nrows` global rows (row r starts at g + r * gstride) into LDS rows of `pitch` bytes: byte b of row r
// lands at r * pitch + (address of the row & 15) + b, so 16-byte units of global memory map to 16-byte units of LDS.
__device__ __forceinline__ void resize_stage_rows(uint8_t* lds, int pitch, const uint8_t* g, size_t gstride, int nrows, int nbytes) {
    const int upr = pitch >> 4;
    for (int i = threadIdx.x; i < nrows * upr; i += RESIZE_THREADS) {
        const int r = i / upr, u = i - r * upr;
        const uint8_t* p = g + (size_t)r * gstride;
        const int b0 = u * 16 - (int)((uintptr_t)p & 15);   // the unit's first byte, relative to the row's first
        if (b0 >= nbytes || b0 + 16 <= 0) continue;
        uint8_t* d = lds + r * pitch + u * 16;
        if (b0 >= 0 && b0 + 16 <= nbytes) {
            *reinterpret_cast<uint4*>(d) = *reinterpret_cast<const uint4*>(p + b0);
        } else {   // head or tail unit: only the bytes of the span
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int b = b0 + j;
                if (b >= 0 && b < nbytes) d[j] = p[b];
            }
        }
    }
}

__device__ __forceinline__ void resize_emit(const ResizeArgs& a, int n, int y, int x, int c0, int c1, int c2) {
    if (a.f32) {
        float* o = static_cast<float*>(a.dst) + ((size_t)n * 3 * a.Hd + y) * a.Wd + x;
        const size_t plane = (size_t)a.Hd * a.Wd;
        o[0] = ((float)c0 / 255.0f - 0.5f) / 0.5f;
        o[plane] = ((float)c1 / 255.0f - 0.5f) / 0.5f;
        o[2 * plane] = ((float)c2 / 255.0f - 0.5f) / 0.5f;
    } else {
        uint8_t* o = static_cast<uint8_t*>(a.dst) + (((size_t)n * a.Hd + y) * a.Wd + x) * 3;
        o[0] = (uint8_t)c0;
        o[1] = (uint8_t)c1;
        o[2] = (uint8_t)c2;
    }
}

template <int MODE>
__global__ void __launch_bounds__(RESIZE_THREADS) k_resize(const ResizeArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t resize_lds[];
    uint8_t* const band = resize_lds;
    uint8_t* const stage = resize_lds + a.band_bytes;

    const int tile_y = blockIdx.x / a.tiles_x, tile_x = blockIdx.x - tile_y * a.tiles_x;
    const int y0 = tile_y * a.TR, x0 = tile_x * a.TC;
    const int rows = min(a.TR, a.Hd - y0), cols = min(a.TC, a.Wd - x0);
    const int c = threadIdx.x & (a.TC - 1);                  // this lane's column of the tile
    const int rsub = threadIdx.x / a.TC, rstep = RESIZE_THREADS / a.TC;
    const int x = x0 + c;
    const bool col_ok = c < cols;

    // the tile's source spans and uniform loop bounds
    int r0 = y0, nband = rows, vmax = 0;
    if (MODE == RM_BOTH || MODE == RM_VONLY) {
        r0 = a.v.bounds[2 * y0];
        nband = a.v.bounds[2 * (y0 + rows - 1)] + a.v.bounds[2 * (y0 + rows - 1) + 1] - r0;
        vmax = a.v.tile_n[tile_y];
    }
    int c0 = x0, nsrc = cols, hmax = 0, hmin = 0, hn = 0;
    if (MODE == RM_BOTH || MODE == RM_HONLY) {
        c0 = a.h.bounds[2 * x0];
        nsrc = a.h.bounds[2 * (x0 + cols - 1)] + a.h.bounds[2 * (x0 + cols - 1) + 1] - c0;
        hmax = a.h.tile_n[tile_x];
        if (col_ok) {
            hmin = a.h.bounds[2 * x];
            hn = a.h.bounds[2 * x + 1];
        }
    }
    const size_t src_row = (size_t)a.Ws * 3;

    for (int n = blockIdx.y; n < a.N; n += gridDim.y) {
        const uint8_t* img = a.src + (size_t)n * a.Hs * src_row;
        if (MODE == RM_COPY) {
            for (int r = rsub; r < rows; r += rstep) {
                if (!col_ok) continue;
                const uint8_t* p = img + (size_t)(y0 + r) * src_row + (size_t)x * 3;
                resize_emit(a, n, y0 + r, x, p[0], p[1], p[2]);
            }
            continue;
        }
        if (MODE == RM_VONLY) {
            resize_stage_rows(band, a.band_pitch, img + (size_t)r0 * src_row + (size_t)c0 * 3, src_row, nband, nsrc * 3);
        } else {
            // horizontal pass over the band's source rows, SR at a time
            for (int b0 = 0; b0 < nband; b0 += a.SR) {
                const int nr = min(a.SR, nband - b0);
                const uint8_t* g = img + (size_t)(r0 + b0) * src_row + (size_t)c0 * 3;
                resize_stage_rows(stage, a.stage_pitch, g, src_row, nr, nsrc * 3);
                __syncthreads();
                for (int r = rsub; r < nr; r += rstep) {
                    if (!col_ok) continue;
                    const int head = (int)((uintptr_t)(g + (size_t)r * src_row) & 15);
                    const uint8_t* s = stage + r * a.stage_pitch + head + (hmin - c0) * 3;
                    int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
                    for (int k = 0; k < hmax; ++k) {
                        if (k < hn) {
                            const int w = a.h.coeffs[(size_t)k * a.Wd + x];
                            acc0 += __mul24((int)s[3 * k], w);
                            acc1 += __mul24((int)s[3 * k + 1], w);
                            acc2 += __mul24((int)s[3 * k + 2], w);
                        }
                    }
                    if (MODE == RM_HONLY) {
                        resize_emit(a, n, y0 + b0 + r, x, resize_clip8(acc0), resize_clip8(acc1), resize_clip8(acc2));
                    } else {
                        uint8_t* d = band + (b0 + r) * a.band_pitch + c * 3;
                        d[0] = (uint8_t)resize_clip8(acc0);
                        d[1] = (uint8_t)resize_clip8(acc1);
                        d[2] = (uint8_t)resize_clip8(acc2);
                    }
                }
                __syncthreads();   // the stage is rewritten by the next chunk (or the next image)
            }
            if (MODE == RM_HONLY) continue;
        }
        // vertical pass out of the band
        if (MODE == RM_VONLY) __syncthreads();
        const uint8_t* g = img + (size_t)r0 * src_row + (size_t)c0 * 3;   // RM_VONLY: where band row 0 came from
        for (int r = rsub; r < rows; r += rstep) {
            if (!col_ok) continue;
            const int y = y0 + r;
            const int vmin = a.v.bounds[2 * y], vn = a.v.bounds[2 * y + 1];
            const int* w = a.v.coeffs + (size_t)y * a.v.ksize;
            int acc0 = 1 << 21, acc1 = 1 << 21, acc2 = 1 << 21;
            for (int k = 0; k < vmax; ++k) {
                if (k < vn) {
                    const int br = vmin - r0 + k;
                    const int head = MODE == RM_VONLY ? (int)((uintptr_t)(g + (size_t)br * src_row) & 15) : 0;
                    const uint8_t* s = band + br * a.band_pitch + head + c * 3;
                    acc0 += __mul24((int)s[0], w[k]);
                    acc1 += __mul24((int)s[1], w[k]);
                    acc2 += __mul24((int)s[2], w[k]);
                }
            }
            resize_emit(a, n, y, x, resize_clip8(acc0), resize_clip8(acc1), resize_clip8(acc2));
        }
        __syncthreads();   // the band is rewritten by the next image
    }
}

}  // namespace cid
