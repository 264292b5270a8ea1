// hash.hpp — the one integer hash of the library: splitmix64's finaliser and what is built on it.  include/srx.h defines
// UMAP's samples, diffmap's start vectors and Harmony's blocks through mix(); synth.hip and the PCA start use the
// generator step.  Host and device: the qualifiers come from the includer (the HIP runtime through common.hpp; a host-only
// program defines __host__, __device__ and __forceinline__ itself).
#pragma once

#include <cstdint>

namespace srx {

constexpr uint64_t kGold64 = 0x9E3779B97F4A7C15ull;      // 2^64 / the golden ratio

// the finaliser alone: srx.h's mix()
__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}
// one step of the generator: the state moves on by kGold64 and is finalised
__host__ __device__ __forceinline__ uint64_t splitmix64(uint64_t x) { return mix64(x + kGold64); }
// the top 53 bits as a double in [0, 1)
__host__ __device__ __forceinline__ double unit53(uint64_t z) { return (double)(z >> 11) * 0x1p-53; }

}  // namespace srx
