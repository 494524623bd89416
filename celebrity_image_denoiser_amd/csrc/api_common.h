// api_common.h — the launch and check plumbing the entry points of cid_api.hip and api/*.h share: the handle base, the images-per-launch split
// and the per-call context with its error text, workspace check and upload check.  Host code only.
#pragma once

#include "../../include/cid.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

namespace cid {

inline int cdiv(int a, int b) { return (a + b - 1) / b; }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
constexpr size_t align64(size_t floats) { return (floats + 63) & ~(size_t)63; }
// An image operand: uint8 NHWC, or fp32 NCHW on a 4-byte boundary.
inline bool fmt_ok(const void* p, int f) { return f == CID_FMT_U8_NHWC || (f == CID_FMT_F32_NCHW && ((uintptr_t)p & 3) == 0); }
// A workspace plan's next region: the offset `at` stands at, which then moves past `bytes`, rounded up to 256.
inline size_t take(size_t& at, size_t bytes) { const size_t o = at; at += align256(bytes); return o; }

// What every handle has: the last error's text and the uploaded (or attached) packed blob.
struct HandleBase {
    std::string err;
    const float* dev_blob = nullptr;
    int fail(int code, const std::string& msg) { err = msg; return code; }
    // The copy of cid_*_upload_weights: `floats` staged floats to `device_blob`, waited for (the staging copy is pageable host memory
    // owned by the handle), then attached as *slot (the handle's blob unless it keeps a second one).  `fn` = "<entry point>: ".
    int upload_blob(const std::string& fn, void* device_blob, const float* staged, size_t floats, void* stream, const float** slot = nullptr) {
        hipStream_t s = static_cast<hipStream_t>(stream);
        hipError_t e = hipMemcpyAsync(device_blob, staged, floats * sizeof(float), hipMemcpyHostToDevice, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return fail(CID_ERR_HIP, fn + hipGetErrorString(e));
        *(slot ? slot : &dev_blob) = static_cast<const float*>(device_blob);
        return CID_OK;
    }
};

// One MFMA convolution layer (3x3, CIN % 8 == 0) in the layout k_disc_conv and k_esd_conv read: cout / part blocks, one per `part`
// output channels, each [CIN/8][9 taps][8][part] weights with its part biases right behind.  Writes the weights (`w`, reference
// [cout][cin][3][3]) or the biases (`b`), whichever is not null, into the layer's segment `seg`.
inline void pack_mfma_layer(float* seg, const float* w, const float* b, int cin, int cout, int part) {
    const size_t nwp = (size_t)cin * 9 * part, block = nwp + part;
    for (int co = 0; co < cout; ++co) {
        float* dst = seg + (size_t)(co / part) * block + co % part;
        if (b) dst[nwp] = b[co];
        for (int ci = 0; w && ci < cin; ++ci)
            for (int tap = 0; tap < 9; ++tap) dst[((size_t)((ci / 8) * 9 + tap) * 8 + ci % 8) * part] = w[((size_t)co * cin + ci) * 9 + tap];
    }
}

// Images per launch: a grid's y (and z) extent ends at 65,535, and the kernels that put one image in a block keep to it in x.
// tests/test_large_batches.py runs every consumer of for_each_launch past it on the smallest images; the other large axis, a tensor
// past 2^31 elements within one launch or across several, is tests/test_wide_offsets.py's.
constexpr int kImagesPerLaunch = 65535;

// launch(n0, images) for each launch of a batch of N images, up to the first one that fails.  Returns hipPeekAtLastError() of that
// launch and leaves the error set: the caller reports it (Call::hip) or returns it, through hipGetLastError(), which clears it.
template <class Launch>
hipError_t for_each_launch(long long N, Launch&& launch) {
    hipError_t e = hipSuccess;
    for (long long n0 = 0; n0 < N && e == hipSuccess; n0 += kImagesPerLaunch) {
        launch((int)n0, (int)std::min<long long>(kImagesPerLaunch, N - n0));
        e = hipPeekAtLastError();
    }
    return e;
}

// cid_*_workspace_bytes / cid_*_saved_bytes: the plan's total where the plan function accepted the shape.
template <class Plan>
int plan_bytes(int rc, const Plan& p, size_t* bytes) {
    if (rc == CID_OK) *bytes = p.total;
    return rc;
}

// One call of entry point `fn` on handle h: its stream, and the checks and the launch error in the entry points' common wording.
struct Call {
    HandleBase* h;
    const char* fn;
    hipStream_t s;
    Call(HandleBase* handle, const char* name, void* stream) : h(handle), fn(name), s(static_cast<hipStream_t>(stream)) {}
    int fail(int code, const std::string& what) const { return h->fail(code, std::string(fn) + ": " + what); }
    // after a failed launch: "<fn>: <what>: <hip error string>"; clears the error
    int hip(const std::string& what) const { return fail(CID_ERR_HIP, what + ": " + hipGetErrorString(hipGetLastError())); }
    // for_each_launch, with the launch that failed reported as hip(what)
    template <class Launch>
    int launches(long long N, const char* what, Launch&& launch) const {
        return for_each_launch(N, launch) == hipSuccess ? CID_OK : hip(what);
    }
    // `buf` (a "workspace", "saved buffer" or "saved arena") holds the `need` bytes that `sizer` reports and is 256-byte aligned
    int room(const void* buf, size_t bytes, size_t need, const char* sizer, const char* noun = "workspace") const {
        if (bytes >= need && !((uintptr_t)buf & 255)) return CID_OK;
        return fail(CID_ERR_WORKSPACE, std::string(noun) + " smaller than " + sizer + "() or not 256-byte aligned");
    }
    int uploaded() const { return h->dev_blob ? CID_OK : fail(CID_ERR_STATE, "weights not uploaded"); }
};

}  // namespace cid
