// Bicubic resize (cid_resize_*): coefficient tables, tile choice and the launch; kernel in resize_kernels.h.  Host code.
#pragma once
#include "../api_common.h"
#include "../resize_kernels.h"

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
