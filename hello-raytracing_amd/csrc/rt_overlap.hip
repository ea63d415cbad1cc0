// rt_overlap.hip — the kernel of rt_overlap_volumes (include/hrt.h rt_overlap_hit): the triangles that touch each of the
// caller's axis-aligned boxes, or the k nearest triangles of each of the caller's points within a radius, in order, and
// the number of all of them, on the triangle tree the other queries read (the host SAH tree of tri_bvh = 1, or the
// device LBVH / PLOC tree, built or refitted). A translation unit of its own: the other code objects do not move.
//
// Shape. One query per lane, 256-lane workgroups, rt_overlap.hpp's query() — the function the host mirror runs — over
// the lane's column of one dynamic LDS block of (24 + 2 k) rows of 256 words: rows 0..23 the walk's stack (as walk_sah,
// the point queries and k_cast_rays_multi keep theirs: a lane's words are all in its own bank, and a wave's 64 lanes read
// 64 consecutive words of a row), rows 24..24+k-1 the list's keys (d2; 0.0f in the box kind, so the same sorted insertion
// orders by index), the next k its triangle indices. 24 KB at k = 0, 26 KB at k = 1, 32 KB at k = 4, 56 KB at k = 16:
// 6, 6, 5 and 2 workgroups on a compute unit's 160 KB. The ball kind's v and w are recomputed for the k winners when the
// records are written.
//
// KIND: RT_VOLUME_BOX or RT_VOLUME_BALL. COUNT_ALL (counts_dev given): every accepted triangle is counted, and the ball
// walk culls by the cap alone; without it the ball walk culls by the list's last d2 once the list is full (the box walk
// has nothing to cull by). STATS: the test-only counting instantiation (include/hrt_testing.h
// rt_testing_set_overlap_count); the product path holds none of its code.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrt.h"
#include "rt_overlap.hpp"
#include "rt_wave_stats.hpp"

using hrt_overlap::Hit;
using hrt_overlap::Launch;

constexpr uint32_t OV_WG = 256u;
static_assert(hrt_overlap::T_MISS == RT_T_MISS, "the shared header's miss value is the public one");
static_assert(hrt_overlap::MAX_K == RT_OVERLAP_MAX_K, "the shared header's capacity is the public one");
static_assert(hrt_overlap::KIND_BOX == RT_VOLUME_BOX && hrt_overlap::KIND_BALL == RT_VOLUME_BALL, "the kinds are the public ones");
static_assert(sizeof(rt_overlap_hit) == sizeof(Hit), "rt_overlap_hit is the shared Hit");

template <uint32_t KIND, bool COUNT_ALL, bool STATS>
__global__ __launch_bounds__(OV_WG) void k_overlap(const Launch A) {
    extern __shared__ uint32_t ov_lds[];  // (STACK + 2 k) rows of OV_WG words
    uint32_t* const stack = ov_lds + threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * OV_WG + threadIdx.x;
    const bool active = i < (uint64_t)A.n;
    hrt_overlap::Tally tally{0u, 0u, 0u};
    if (active) {
        constexpr uint32_t W = KIND == hrt_overlap::KIND_BOX ? 6u : 4u;
        float vol[W];
#pragma unroll
        for (uint32_t c = 0; c < W; c++) vol[c] = A.volumes[W * i + c];
        const bool cur = A.after != nullptr;  // (d2 and prim only; 4-byte aligned)
        const float after_d2 = cur ? A.after[i].d2 : 0.0f;
        const int32_t after_j = cur ? A.after[i].prim : -1;
        hrt_overlap::List L;
        L.lt = (float*)(stack + hrt_overlap::STACK * OV_WG);
        L.lj = (int32_t*)(stack + (hrt_overlap::STACK + A.k) * OV_WG);
        L.stride = OV_WG;
        L.k = A.k;
        L.n = 0u;
        uint32_t count = 0u;
        hrt_overlap::query<KIND, COUNT_ALL, STATS>(A.tree, vol, cur, after_d2, after_j, stack, OV_WG, L, count, tally);
        uint4* const out = (uint4*)A.hits + i * A.k;
        for (uint32_t s = 0; s < A.k; s++) {
            const Hit h = hrt_overlap::make_record<KIND>(A.tree, vol, L, s);
            out[s] = uint4{__float_as_uint(h.d2), (uint32_t)h.prim, __float_as_uint(h.v), __float_as_uint(h.w)};
        }
        if constexpr (COUNT_ALL) A.counts[i] = count;
    }
    if constexpr (STATS) {  // per wave: four sums, one agent-scope add per word (every lane of the wave is here)
        hrt_wave::wave_add<4>(A.stats, {active ? 1ull : 0ull, tally.tri, tally.box, tally.overflow});
    }
}

template <uint32_t KIND>
static void launch_kind(const Launch& a, bool stats, uint32_t blocks, size_t lds, hipStream_t stream) {
    const bool all = a.counts != nullptr;
    if (all && stats) hipLaunchKernelGGL((k_overlap<KIND, true, true>), dim3(blocks), dim3(OV_WG), lds, stream, a);
    else if (all) hipLaunchKernelGGL((k_overlap<KIND, true, false>), dim3(blocks), dim3(OV_WG), lds, stream, a);
    else if (stats) hipLaunchKernelGGL((k_overlap<KIND, false, true>), dim3(blocks), dim3(OV_WG), lds, stream, a);
    else hipLaunchKernelGGL((k_overlap<KIND, false, false>), dim3(blocks), dim3(OV_WG), lds, stream, a);
}

hipError_t hrt_launch_overlap(const Launch& a, bool stats, hipStream_t stream) {
    if (a.n == 0u) return hipSuccess;
    if (a.kind != hrt_overlap::KIND_BOX && a.kind != hrt_overlap::KIND_BALL) return hipErrorInvalidValue;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + OV_WG - 1u) / OV_WG);
    const size_t lds = (size_t)(hrt_overlap::STACK + 2u * a.k) * OV_WG * sizeof(uint32_t);
    if (a.kind == hrt_overlap::KIND_BOX) launch_kind<hrt_overlap::KIND_BOX>(a, stats, blocks, lds, stream);
    else launch_kind<hrt_overlap::KIND_BALL>(a, stats, blocks, lds, stream);
    return hipGetLastError();
}
