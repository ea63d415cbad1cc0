// rt_closest.hip — the kernel of rt_closest_points (include/hrt.h rt_closest): the nearest point of the triangle set for
// each of the caller's points, on the triangle tree the ray walks read (the host SAH tree of tri_bvh = 1, or the device
// LBVH / PLOC tree, built or refitted). A translation unit of its own: rt_kernels.hip's, rt_regroup.hip's, rt_lbvh.hip's and
// rt_ploc.hip's code objects do not move.
//
// Shape. One query per lane, 256-lane workgroups, an ordered culling stack walk of the two-child nodes (32 B: per child
// six halves relative to the root centre and the child word). Per node both children's boxes are decoded (half to float
// is exact) and a lower bound lb2 of the squared distance from the point to each box, taken `pad` closer than the box
// stands, is compared with the best squared distance so far: a child is visited unless lb2 > best (equality visits: an
// equal distance at a smaller index replaces the answer), the nearer child first, the other one on the stack. Leaves hold
// up to 15 entries of tb_order, each tested with rt_closest.hpp's point_triangle — the function the host definition
// loops over all triangles, so a walk that skips nothing the definition would accept returns its bytes.
//
// The stack: STACK = 24 words per lane in LDS at stride 256 (24 KB per workgroup: 6 workgroups, 24 waves per compute unit;
// a popped word's bank is the lane's, no conflicts), as walk_sah keeps its own. A PLOC tree may be 64 deep: a subtree that
// does not fit is dropped and flagged, and the query finishes with the loop over all m triangles — the definition itself,
// started from the walk's answer (a lexicographic minimum does not depend on the order of its candidates).
//
// Coverage. The bound holds for finite points with D = |p - rc| * 1.001 + rr_h in [2^-40, 2^60]; any
// other point (NaN and infinite ones fail the same comparison) takes the loop over all triangles instead of the walk.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrt.h"
#include "rt_closest.hpp"
#include "rt_wave_stats.hpp"

using hrt_closest::Launch;
using hrt_closest::Record;
using hrt_closest::U4;

constexpr uint32_t CP_WG = 256u;
static_assert(hrt_closest::T_MISS == RT_T_MISS, "the shared header's miss value is the public one");
static_assert(sizeof(rt_closest) == sizeof(Record), "rt_closest is the shared Record");

// COUNT: the test-only counting instantiation (include/hrt_testing.h rt_testing_set_closest_count); the product path
// launches COUNT = false, which holds none of the counting code.
template <bool COUNT>
__global__ __launch_bounds__(CP_WG) void k_closest_points(const Launch A) {
    __shared__ uint32_t stack_lds[hrt_closest::STACK * CP_WG];
    uint32_t* const stack = stack_lds + threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * CP_WG + threadIdx.x;
    const bool active = i < (uint64_t)A.n;
    uint32_t tests = 0u, overflow = 0u, uncovered = 0u;
    if (active) {
        const float p[3] = {A.points[3 * i], A.points[3 * i + 1], A.points[3 * i + 2]};
        float best = hrt_closest::cap_of(A.maxd2 != nullptr ? A.maxd2[i] : hrt_closest::T_MISS), bv = 0.0f, bw = 0.0f;
        int32_t bj = -1;
        if (best > 0.0f) {
            const float q[3] = {p[0] - A.rc[0], p[1] - A.rc[1], p[2] - A.rc[2]};
            const float D = __builtin_sqrtf(hrt_closest::dot3(q, q)) * 1.001f + A.rr_h;
            const bool covered = D >= hrt_closest::D_MIN && D <= hrt_closest::D_MAX;
            if (covered) {
                const float pad = D * hrt_closest::PAD;
                uint32_t node = A.root;
                int sp = 0;
                while (true) {
                    if (!(node & hrt_closest::LEAF_BIT)) {
                        const U4 L = A.hnodes[2 * (size_t)node], R = A.hnodes[2 * (size_t)node + 1];
                        const float ll = hrt_closest::box_lb2(L, q, pad), lr = hrt_closest::box_lb2(R, q, pad);
                        const bool vl = !(ll > best), vr = !(lr > best);
                        if (vl && vr) {
                            const bool lfirst = ll <= lr;
                            if (sp < hrt_closest::STACK) {
                                stack[sp * CP_WG] = lfirst ? R.w : L.w;
                                sp++;
                            } else {
                                overflow = 1u;
                            }
                            node = lfirst ? L.w : R.w;
                            continue;
                        }
                        if (vl) { node = L.w; continue; }
                        if (vr) { node = R.w; continue; }
                    } else {
                        const uint32_t first = (node >> 4) & 0x07FFFFFFu, cnt = node & 15u;
                        for (uint32_t k = 0; k < cnt; k++)
                            hrt_closest::test_triangle(p, A.geo, A.order[first + k], best, bj, bv, bw);
                        if constexpr (COUNT) tests += cnt;
                    }
                    if (sp == 0) break;
                    node = stack[(--sp) * CP_WG];
                }
            } else {
                uncovered = 1u;
            }
            if (!covered || overflow != 0u) {  // the definition: every triangle (NaN and non-finite ones are never accepted)
                for (uint32_t j = 0; j < A.m; j++) hrt_closest::test_triangle(p, A.geo, j, best, bj, bv, bw);
                if constexpr (COUNT) tests += A.m;
            }
        }
        const Record rec = hrt_closest::make_record(A.geo, best, bj, bv, bw);
        uint4* const o = (uint4*)A.out + 2 * i;
        o[0] = uint4{__float_as_uint(rec.d2), (uint32_t)rec.prim, __float_as_uint(rec.p[0]), __float_as_uint(rec.p[1])};
        o[1] = uint4{__float_as_uint(rec.p[2]), __float_as_uint(rec.v), __float_as_uint(rec.w), 0u};
    }
    if constexpr (COUNT) {  // per wave: four sums, one agent-scope add per word (every lane of the wave is here)
        hrt_wave::wave_add<4>(A.counts, {active ? 1ull : 0ull, tests, overflow, uncovered});
    }
}

hipError_t hrt_launch_closest(const Launch& a, bool count, hipStream_t stream) {
    if (a.n == 0u) return hipSuccess;
    const uint32_t blocks = (uint32_t)(((uint64_t)a.n + CP_WG - 1u) / CP_WG);
    if (count) hipLaunchKernelGGL(k_closest_points<true>, dim3(blocks), dim3(CP_WG), 0, stream, a);
    else hipLaunchKernelGGL(k_closest_points<false>, dim3(blocks), dim3(CP_WG), 0, stream, a);
    return hipGetLastError();
}
