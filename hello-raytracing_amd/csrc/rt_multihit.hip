// rt_multihit.hip — the kernel of rt_cast_rays_multi (include/hrt.h rt_multi_hit): the k nearest hits along each of the
// caller's rays, in order, and the number of all of them, on the triangle tree the other queries read (the host SAH tree
// of tri_bvh = 1, or the device LBVH / PLOC tree, built or refitted). A translation unit of its own: the other code
// objects do not move.
//
// Shape. One ray per lane, 256-lane workgroups, rt_multihit.hpp's query() — the function the host mirror runs — over
// the lane's column of one dynamic LDS block of (24 + 2 k) rows of 256 words: rows 0..23 the walk's stack (as walk_sah
// and the point queries keep theirs: a lane's words are all in its own bank), rows 24..24+k-1 the list's t, the next k
// its triangle indices. 24 KB at k = 0, 26 KB at k = 1, 32 KB at k = 4, 56 KB at k = 16: 6, 6, 5 and 2 workgroups on a
// compute unit's 160 KB. u and v are recomputed for the k winners when the records are written.
//
// COUNT_ALL (counts_dev given): the walk culls by the cap alone and counts every accepted triangle; without it the walk
// culls by the list's last t once the list is full. STATS: the test-only counting instantiation (include/hrt_testing.h
// rt_testing_set_multihit_count); the product path holds none of its code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrt.h"
#include "rt_multihit.hpp"
#include "rt_wave_stats.hpp"

using hrt_multihit::Hit;
using hrt_multihit::Launch;

constexpr uint32_t MH_WG = 256u;
static_assert(hrt_multihit::T_MISS == RT_T_MISS, "the shared header's miss value is the public one");
static_assert(hrt_multihit::MAX_K == RT_MULTI_HIT_MAX_K, "the shared header's capacity is the public one");
static_assert(sizeof(rt_multi_hit) == sizeof(Hit), "rt_multi_hit is the shared Hit");

template <bool COUNT_ALL, bool STATS>
__global__ __launch_bounds__(MH_WG) void k_cast_rays_multi(const Launch A) {
    extern __shared__ uint32_t mh_lds[];  // (STACK + 2 k) rows of MH_WG words
    uint32_t* const stack = mh_lds + threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * MH_WG + threadIdx.x;
    const bool active = i < (uint64_t)A.n;
    hrt_multihit::Tally tally{0u, 0u, 0u};
    if (active) {
        const float o[3] = {A.origins[3 * i], A.origins[3 * i + 1], A.origins[3 * i + 2]};
        const float d[3] = {A.dirs[3 * i], A.dirs[3 * i + 1], A.dirs[3 * i + 2]};
        const float tmax = A.tmax != nullptr ? A.tmax[i] : hrt_multihit::T_MISS;
        const bool cur = A.after != nullptr;  // (t and prim only; 4-byte aligned)
        const float after_t = cur ? A.after[i].t : 0.0f;
        const int32_t after_j = cur ? A.after[i].prim : -1;
        hrt_multihit::List L;
        L.lt = (float*)(stack + hrt_multihit::STACK * MH_WG);
        L.lj = (int32_t*)(stack + (hrt_multihit::STACK + A.k) * MH_WG);
        L.stride = MH_WG;
        L.k = A.k;
        L.n = 0u;
        uint32_t count = 0u;
        hrt_multihit::query<COUNT_ALL, STATS>(A.tree, o, d, tmax, cur, after_t, after_j, stack, MH_WG, L, count, tally);
        uint4* const out = (uint4*)A.hits + i * A.k;
        for (uint32_t s = 0; s < A.k; s++) {
            const Hit h = hrt_multihit::make_record(A.tree, o, d, L, s);
            out[s] = uint4{__float_as_uint(h.t), (uint32_t)h.prim, __float_as_uint(h.u), __float_as_uint(h.v)};
        }
        if constexpr (COUNT_ALL) A.counts[i] = count;
    }
    if constexpr (STATS) {  // per wave: four sums, one agent-scope add per word (every lane of the wave is here)
        hrt_wave::wave_add<4>(A.stats, {active ? 1ull : 0ull, tally.tri, tally.box, tally.overflow});
    }
}

hipError_t hrt_launch_multihit(const Launch& a, bool stats, hipStream_t stream) {
    if (a.n == 0u) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + MH_WG - 1u) / MH_WG);
    const size_t lds = (size_t)(hrt_multihit::STACK + 2u * a.k) * MH_WG * sizeof(uint32_t);
    const bool all = a.counts != nullptr;
    if (all && stats) hipLaunchKernelGGL((k_cast_rays_multi<true, true>), dim3(blocks), dim3(MH_WG), lds, stream, a);
    else if (all) hipLaunchKernelGGL((k_cast_rays_multi<true, false>), dim3(blocks), dim3(MH_WG), lds, stream, a);
    else if (stats) hipLaunchKernelGGL((k_cast_rays_multi<false, true>), dim3(blocks), dim3(MH_WG), lds, stream, a);
    else hipLaunchKernelGGL((k_cast_rays_multi<false, false>), dim3(blocks), dim3(MH_WG), lds, stream, a);
    return hipGetLastError();
}
