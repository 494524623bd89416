// hash_streams.h — the counter-based splitmix64 streams of synth.py on the device, shared by every kernel that draws from them
// (noise_kernels.h, cgan_kernels.h): element e of stream `id` under seed s is z = splitmix64(splitmix64(s ^ id) + e),
// u = (z >> 11) * 2^-53, and a normal deviate is Box-Muller of two such streams in float64, in numpy's evaluation order with
// contraction off.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cid {

constexpr uint64_t fnv1a64(const char* s, uint64_t h = 0xCBF29CE484222325ull) {
    return *s ? fnv1a64(s + 1, (h ^ (uint64_t)(unsigned char)*s) * 0x100000001B3ull) : h;
}

__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__device__ __forceinline__ double unit_double(uint64_t z) {
#pragma clang fp contract(off)
    return (double)(z >> 11) * (1.0 / 9007199254740992.0);
}

// sqrt(-2*log(1-u1)) * cos((2*pi)*u2), numpy's evaluation order
__device__ __forceinline__ double box_muller(double u1, double u2) {
#pragma clang fp contract(off)
    return sqrt(-2.0 * log(1.0 - u1)) * cos(6.283185307179586 * u2);
}

}  // namespace cid
