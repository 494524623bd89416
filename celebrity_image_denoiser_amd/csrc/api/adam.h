// The optimizer step (cid_adam_step): argument checks and the launch; kernel in optim_kernels.h.  Host code.
#pragma once
#include "../api_common.h"
#include "../optim_kernels.h"

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
