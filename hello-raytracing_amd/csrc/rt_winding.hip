// rt_winding.hip — the kernels of rt_winding_numbers (include/hrt.h): the generalized winding number of the triangle set
// at each of the caller's points, on the triangle tree the ray walks read (the host SAH tree of tri_bvh = 1, or the device
// LBVH / PLOC tree, built or refitted), and the moments of that tree's subtrees. A translation unit of its own:
// rt_kernels.hip's, rt_regroup.hip's, rt_lbvh.hip's, rt_ploc.hip's and rt_closest.hip's code objects do not move.
//
// k_winding. One query per lane, 256-lane workgroups; the whole query is rt_winding.hpp's query(), the function the host
// mirror runs, so the device returns its bytes. One loop body judges one child of one node by the far-field rule, from its
// packed box and its 32-byte half of the node's moment record: a far child is one dipole term, a near leaf is summed
// triangle by triangle, a near node is descended; a node whose left child is descended waits on the stack for its right
// one. The stack: STACK = 24 words per lane in LDS at stride 256 (24 KB per workgroup; a popped word's bank is the lane's,
// no conflicts), as k_closest_points keeps it. A query that needs more, a point outside the covered range and a tree
// without nodes take the loop over all m triangles.
//
// k_tree_moments. One lane per node slot. A referenced node's lane sums its leaf children (their order entries in order, in
// f64) into the (node, side) slots of the scratch and adds their number to the node's arrival counter; the lane whose
// add brings the counter to 2 reads both slots, writes the node's record, and carries left + right to the slot of its
// side at the parent (tb_parent), where the same rule applies. No lane waits, spins or polls. The hand-off is
// k_lbvh_fit's: agent-scope atomic stores of the slot, s_waitcnt vmcnt(0), the agent-scope arrival add, agent-scope atomic
// loads of both slots after the add has returned. left + right is one IEEE addition per word: which lane arrives second
// changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrt.h"
#include "rt_wave_stats.hpp"
#include "rt_winding.hpp"

using hrt_winding::Launch;
using hrt_winding::MomentsLaunch;
using hrt_winding::Sums;
using hrt_winding::U4;

constexpr uint32_t WN_WG = 256u;
#define HRT_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// COUNT: the test-only counting instantiation (include/hrt_testing.h rt_testing_set_winding_count); the product path
// launches COUNT = false, which holds none of the counting code.
template <bool COUNT>
__global__ __launch_bounds__(WN_WG) void k_winding(const Launch A) {
    __shared__ uint32_t stack_lds[hrt_winding::STACK * WN_WG];
    const uint64_t i = (uint64_t)blockIdx.x * WN_WG + threadIdx.x;
    const bool active = i < (uint64_t)A.n;
    hrt_winding::Tally t{0u, 0u, 0u, 0u};
    if (active) {
        const float p[3] = {A.points[3 * i], A.points[3 * i + 1], A.points[3 * i + 2]};
        A.out[i] = hrt_winding::query<COUNT>(A.tree, p, A.beta, stack_lds + threadIdx.x, WN_WG, t);
    }
    if constexpr (COUNT) {  // per wave: five sums, one agent-scope add per word (every lane of the wave is here)
        hrt_wave::wave_add<5>(A.counts, {active ? 1ull : 0ull, t.tri, t.dip, t.overflow, t.uncovered});
    }
}

static __device__ inline void store_sums(unsigned long long* slot, const Sums& a) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        __hip_atomic_store(&slot[k], (unsigned long long)__double_as_longlong(a.N[k]), HRT_RLX_AGENT);
        __hip_atomic_store(&slot[3 + k], (unsigned long long)__double_as_longlong(a.G[k]), HRT_RLX_AGENT);
    }
    __hip_atomic_store(&slot[6], (unsigned long long)__double_as_longlong(a.s), HRT_RLX_AGENT);
}
static __device__ inline void load_sums(unsigned long long* slot, Sums& a) {
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.N[k] = __longlong_as_double((long long)__hip_atomic_load(&slot[k], HRT_RLX_AGENT));
        a.G[k] = __longlong_as_double((long long)__hip_atomic_load(&slot[3 + k], HRT_RLX_AGENT));
    }
    a.s = __longlong_as_double((long long)__hip_atomic_load(&slot[6], HRT_RLX_AGENT));
}

__global__ __launch_bounds__(WN_WG) void k_tree_moments(const MomentsLaunch a) {
    const uint32_t i = blockIdx.x * WN_WG + threadIdx.x;
    if (i >= a.slots) return;
    uint32_t node = i;
    U4 box[2] = {a.hnodes[2u * (size_t)node], a.hnodes[2u * (size_t)node + 1u]};
    if (box[0].w == 0u) return;  // a slot no child word names (k_lbvh_fit's test)
    uint32_t added = 0u;
    for (uint32_t s = 0; s < 2u; s++) {
        if ((box[s].w & hrt_winding::LEAF_BIT) == 0u) continue;
        Sums leaf;
        hrt_winding::leaf_sums(box[s].w, a.order, a.geo, a.rc, leaf);
        store_sums(a.sums + (2u * (size_t)node + s) * hrt_winding::SUM_WORDS, leaf);
        added++;
    }
    if (added == 0u) return;  // both children are nodes: the second of them to arrive goes on from here
    // (at most 64 levels above a leaf: rt_lbvh.hpp, the level cap of the fit kernels)
    for (uint32_t level = 0; level <= 64u; level++) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slot's stores are complete before the arrival counts
        const uint32_t before = __hip_atomic_fetch_add(&a.arrivals[node], added, HRT_RLX_AGENT);
        asm volatile("" ::: "memory");  // (the slot loads below stay below the add)
        if (before + added < 2u) return;  // the other side is still to come: its lane takes this one along
        Sums side[2];
        load_sums(a.sums + (2u * (size_t)node) * hrt_winding::SUM_WORDS, side[0]);
        load_sums(a.sums + (2u * (size_t)node + 1u) * hrt_winding::SUM_WORDS, side[1]);
        float rec[hrt_winding::REC_FLOATS];
        hrt_winding::child_record(side[0], box[0], rec);
        hrt_winding::child_record(side[1], box[1], rec + 8);
        float4* const o = (float4*)(a.moments + hrt_winding::REC_FLOATS * (size_t)node);
#pragma unroll
        for (int k = 0; k < 4; k++) o[k] = float4{rec[4 * k], rec[4 * k + 1], rec[4 * k + 2], rec[4 * k + 3]};
        hrt_winding::sums_add(side[0], side[1]);
        const uint32_t link = a.parent[node];
        if (link == hrt_winding::NO_PARENT) return;
        const uint32_t up = link >> 1, s = link & 1u;
        if (up >= a.slots) return;  // (never: a link names a node slot)
        store_sums(a.sums + (2u * (size_t)up + s) * hrt_winding::SUM_WORDS, side[0]);
        node = up;
        added = 1u;
        box[0] = a.hnodes[2u * (size_t)node];
        box[1] = a.hnodes[2u * (size_t)node + 1u];
    }
}

hipError_t hrt_launch_winding(const Launch& a, bool count, hipStream_t stream) {
    if (a.n == 0u) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + WN_WG - 1u) / WN_WG);
    if (count) hipLaunchKernelGGL(k_winding<true>, dim3(blocks), dim3(WN_WG), 0, stream, a);
    else hipLaunchKernelGGL(k_winding<false>, dim3(blocks), dim3(WN_WG), 0, stream, a);
    return hipGetLastError();
}

// slots > 0. The arrival counters are zeroed here on every call.
hipError_t hrt_launch_tree_moments(const MomentsLaunch& a, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(a.arrivals, 0, (size_t)a.slots * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.moments, 0, (size_t)a.slots * hrt_winding::REC_FLOATS * sizeof(float), stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_tree_moments, dim3((a.slots + WN_WG - 1u) / WN_WG), dim3(WN_WG), 0, stream, a);
    return hipGetLastError();
}
