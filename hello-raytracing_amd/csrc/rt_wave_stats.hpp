// rt_wave_stats.hpp — the epilogue of the tree queries' counting instantiations (include/hrt_testing.h), device code only:
// every lane of a wave brings N values (an inactive lane brings zeros), the wave sums each, and lane 0 adds the N sums to
// N counter words with relaxed agent-scope atomics. A product instantiation calls none of it.
#pragma once
#include <hip/hip_runtime.h>

namespace hrt_wave {

static __device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Every lane of the wave must be here (the sums are cross-lane shuffles).
template <int N>
static __device__ inline void wave_add(unsigned long long* words, const unsigned long long (&v)[N]) {
    unsigned long long s[N];
#pragma unroll
    for (int k = 0; k < N; k++) s[k] = wave_sum(v[k]);
    if ((threadIdx.x & 63u) == 0u) {
#pragma unroll
        for (int k = 0; k < N; k++) __hip_atomic_fetch_add(&words[k], s[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

}  // namespace hrt_wave
