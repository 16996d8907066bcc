// The order-preserving 32-bit key of a float that K30 (robust_images.hip) and K31 (running_baseline.hip) select on;
// tests/robust_restatement.py R1 is its definition.
#pragma once

#include <cstdint>

#include "common.hpp"

namespace dnmf {

// value -> key with key(a) < key(b) <=> a < b for finite a, b; -0 and +0 share the key of +0
__device__ __forceinline__ uint32_t to_key32(float v) {
    const uint32_t u = v == 0.0f ? 0u : __float_as_uint(v);
    return (u >> 31) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float from_key32(uint32_t k) { return __uint_as_float((k >> 31) ? (k & 0x7fffffffu) : ~k); }

}  // namespace dnmf
