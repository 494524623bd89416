// weight_store.h — the host-side weight staging the model handles of api/*.h share (cid_esr_*, cid_sr_*, cid_cg_*, cid_lpips_*,
// cid_vgg_*): the key table, the tensors as they were set and the packed blob's staging copy, over HandleBase.  Host code only.
//
// A handle struct derives from WeightStore and adds its few own fields; its extern "C" functions are a few lines over the store.  A
// new model supplies a key table (KeyTable), a pack step (the staged tensors -> the kernels' layout) and its own fields and forward.
#pragma once

#include "api_common.h"

#include <cmath>
#include <initializer_list>
#include <string>
#include <utility>
#include <vector>

namespace cid {

struct WeightKey {
    std::string name;
    int64_t shape[4];
    int ndim;
    size_t count;
    bool counter;   // num_batches_tracked: part of the state_dict, a 0-d tensor, accepted and unused in eval mode
};

// A key table in state_dict order.
struct KeyTable : std::vector<WeightKey> {
    void tensor(const std::string& name, std::initializer_list<int64_t> shape) {
        WeightKey k{name, {0, 0, 0, 0}, (int)shape.size(), 1, false};
        std::copy(shape.begin(), shape.end(), k.shape);
        for (const int64_t d : shape) k.count *= (size_t)d;
        push_back(k);
    }
    void conv(const std::string& prefix, int co, int ci, int ks) {   // Conv2d: <prefix>weight, <prefix>bias
        tensor(prefix + "weight", {co, ci, ks, ks});
        tensor(prefix + "bias", {co});
    }
    void batchnorm(const std::string& prefix, int c) {               // BatchNorm2d(affine=True, track_running_stats=True)
        for (const char* leaf : {"weight", "bias", "running_mean", "running_var"}) tensor(prefix + leaf, {c});
        push_back({prefix + "num_batches_tracked", {0, 0, 0, 0}, 0, 1, true});
    }
};

struct WeightStore : HandleBase {
    std::string prefix;                    // the family's name in every message: "cid_esr", ...
    std::vector<WeightKey> keys;
    std::vector<std::vector<float>> raw;   // the tensors as set, reference layout
    std::vector<char> have;
    std::vector<float> staging;            // the packed blob; pageable host memory owned by the handle

    void init(const char* family, std::vector<WeightKey> table) {
        prefix = family;
        keys = std::move(table);
        raw.resize(keys.size());
        have.assign(keys.size(), 0);
    }

    int find(const std::string& k) const {
        for (size_t i = 0; i < keys.size(); ++i)
            if (keys[i].name == k) return (int)i;
        return -1;
    }

    const float* get(const std::string& k) const { return raw[find(k)].data(); }

    const char* key(int i) const { return i < 0 || (size_t)i >= keys.size() ? nullptr : keys[i].name.c_str(); }

    // cid_*_set_weight
    int set(const char* key, const void* data, const int64_t* shape, int ndim) {
        const std::string fn = prefix + "_set_weight: ";
        if (!key || !data || (!shape && ndim > 0)) return fail(CID_ERR_INVALID, fn + "null argument");
        const int i = find(key);
        if (i < 0) return fail(CID_ERR_KEY, fn + "unexpected key '" + key + "'");
        const WeightKey& k = keys[i];
        if (ndim != k.ndim || !std::equal(shape, shape + ndim, k.shape)) return fail(CID_ERR_SHAPE, fn + "size mismatch for " + k.name);
        if (!k.counter) {
            const float* f = static_cast<const float*>(data);
            raw[i].assign(f, f + k.count);
        }
        have[i] = 1;
        return CID_OK;
    }

    // cid_*_set_bn_eps; `slot` is null where the handle has no such BatchNorm
    int set_bn_eps(double* slot, double eps) {
        if (!slot) return fail(CID_ERR_INVALID, prefix + "_set_bn_eps: no such BatchNorm");
        if (!std::isfinite(eps) || eps < 0.0) return fail(CID_ERR_INVALID, prefix + "_set_bn_eps: eps must be finite and >= 0");
        *slot = eps;
        return CID_OK;
    }

    // the index of the first tensor the pack step needs and does not have, or -1
    int first_missing() const {
        for (size_t i = 0; i < keys.size(); ++i)
            if (!keys[i].counter && !have[i]) return (int)i;
        return -1;
    }

    int missing() const {
        int m = 0;
        for (size_t i = 0; i < keys.size(); ++i) m += !keys[i].counter && !have[i];
        return m;
    }

    // cid_*_upload_weights: the checks, pack(staging) over a zeroed blob of `blob_floats`, the copy.  `complete` = false leaves the
    // check that every tensor is set to the caller (cid_vgg_upload_weights has its own, which it runs first).
    template <class Pack>
    int upload(void* device_blob, void* stream, size_t blob_floats, Pack pack, bool complete = true) {
        const std::string fn = prefix + "_upload_weights: ";
        if (!device_blob) return fail(CID_ERR_INVALID, fn + "null device pointer");
        if ((uintptr_t)device_blob & 255) return fail(CID_ERR_WORKSPACE, fn + "blob must be 256-byte aligned");
        if (complete && first_missing() >= 0) return fail(CID_ERR_STATE, fn + keys[first_missing()].name + " not set");
        staging.assign(blob_floats, 0.f);
        pack(staging.data());
        return upload_blob(fn, device_blob, staging.data(), staging.size(), stream);
    }
};

}  // namespace cid
