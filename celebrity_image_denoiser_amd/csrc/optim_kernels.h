// optim_kernels.h — the trainer's optimizer step (torch.optim.Adam with default flags, training.py:239-240) on the device.
//
// k_adam_step updates every tensor of one optimizer in ONE launch: up to ADAM_MAX_TENSORS entries (param, grad, exp_avg, exp_avg_sq,
// count) lie in the kernel arguments with a prefix of work items, and a workgroup finds its tensor by binary search in that table,
// the way k_gen_pack finds its segment.  The work item is blockIdx.x, so the entry and everything read from it stay in scalar
// registers.
//
// Form: a lane owns one quad of four consecutive elements, a workgroup ADAM_THREADS consecutive quads of ONE tensor.  The ABI
// promises 4-byte alignment only.  Where a tensor's four pointers share their offset within 16 bytes (every tensor a torch
// allocation starts does), the quad grid is shifted by `off` phantom elements in front of the tensor so that quads start on 16-byte
// boundaries: the inner quads move as one 16-byte load per operand and one 16-byte store per result, the first and the last
// quad of the tensor (the 4-byte head and tail) element by element.  Where the four pointers disagree, off = 0 and every quad goes
// element by element.  Element e of a tensor belongs to exactly one (quad, word) = ((e + off) / 4, (e + off) % 4), so every element of
// param, exp_avg and exp_avg_sq is written exactly once; nothing is read after it is written, grad is only read; no LDS, no atomics.
//
// Arithmetic (the contract of cid_adam_step, include/cid.h; synth.adam_step_np restates it in numpy): double from the fp32 operands,
// no contraction, one rounding per stored value.  lr / bc1 and sqrt(bc2) depend on the tensor only and come from the host in double.
// All of it is __host__ __device__: cid_debug_adam_step_host runs the same table and work-item code on the CPU over host pointers, so
// the index arithmetic and the expression tree are tested without a GPU (tests/test_adam_host.py).
#pragma once
#include <hip/hip_runtime.h>

namespace cid {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_MAX_TENSORS = 32;          // CID_ADAM_MAX_TENSORS
constexpr int ADAM_ITEM_ELEMS = 4 * ADAM_THREADS;

struct AdamEntry {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    long long count;       // elements, > 0 (the host leaves empty tensors out)
    unsigned t0;           // work items of the entries before this one
    unsigned off;          // phantom elements in front of element 0 (0..3); ADAM_SCALAR: the four pointers disagree, off = 0, no 16-byte access
    double step_size;      // lr / (1 - beta1^t)
    double bc2_sqrt;       // sqrt(1 - beta2^t)
};
constexpr unsigned ADAM_SCALAR = 4;

struct AdamArgs {
    double beta1, one_minus_beta1, beta2, one_minus_beta2, eps, weight_decay;
    unsigned nitems;
    int nent;
    AdamEntry ent[ADAM_MAX_TENSORS];
};

// One element: p, m, v are updated in place in the caller's registers.
__host__ __device__ inline void adam_element(const AdamArgs& a, const AdamEntry& s, float& p, float gf, float& m, float& v) {
#pragma clang fp contract(off)
    double g = (double)gf;
    if (a.weight_decay != 0.0) g = g + a.weight_decay * (double)p;
    m = (float)((double)m * a.beta1 + a.one_minus_beta1 * g);
    v = (float)((double)v * a.beta2 + (a.one_minus_beta2 * g) * g);
    const double denom = __builtin_sqrt((double)v) / s.bc2_sqrt + a.eps;
    p = (float)((double)p - s.step_size * ((double)m / denom));
}

// Work item `item` (workgroup-uniform) as seen by lane `tid` of its workgroup.
__host__ __device__ inline void adam_item(const AdamArgs& a, unsigned item, unsigned tid) {
    if (item >= a.nitems) return;
    int lo = 0, hi = a.nent - 1;   // the last entry that starts at or before the item
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (a.ent[mid].t0 <= item) lo = mid;
        else hi = mid - 1;
    }
    const AdamEntry& s = a.ent[lo];
    const bool vec = s.off != ADAM_SCALAR;
    const long long e0 = 4 * ((long long)(item - s.t0) * ADAM_THREADS + tid) - (vec ? (long long)s.off : 0);
    if (e0 >= s.count) return;
    float* __restrict__ P = s.param;
    const float* __restrict__ G = s.grad;
    float* __restrict__ M = s.exp_avg;
    float* __restrict__ V = s.exp_avg_sq;
    if (vec && e0 >= 0 && e0 + 4 <= s.count) {
        float4 p = *reinterpret_cast<const float4*>(P + e0);
        const float4 g = *reinterpret_cast<const float4*>(G + e0);
        float4 m = *reinterpret_cast<const float4*>(M + e0);
        float4 v = *reinterpret_cast<const float4*>(V + e0);
        adam_element(a, s, p.x, g.x, m.x, v.x);
        adam_element(a, s, p.y, g.y, m.y, v.y);
        adam_element(a, s, p.z, g.z, m.z, v.z);
        adam_element(a, s, p.w, g.w, m.w, v.w);
        *reinterpret_cast<float4*>(M + e0) = m;
        *reinterpret_cast<float4*>(V + e0) = v;
        *reinterpret_cast<float4*>(P + e0) = p;
        return;
    }
    // head, tail, or a tensor whose pointers do not share an alignment: 4-byte accesses.  All loads first, as above.
    float p[4], g[4], m[4], v[4];
    bool in[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long long e = e0 + k;
        in[k] = e >= 0 && e < s.count;
        if (in[k]) { p[k] = P[e]; g[k] = G[e]; m[k] = M[e]; v[k] = V[e]; }
        else { p[k] = g[k] = m[k] = v[k] = 0.0f; }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!in[k]) continue;
        adam_element(a, s, p[k], g[k], m[k], v[k]);
        M[e0 + k] = m[k];
        V[e0 + k] = v[k];
        P[e0 + k] = p[k];
    }
}

__global__ void __launch_bounds__(ADAM_THREADS) k_adam_step(const AdamArgs a) { adam_item(a, blockIdx.x, threadIdx.x); }

}  // namespace cid
