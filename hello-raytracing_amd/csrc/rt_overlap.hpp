// rt_overlap.hpp — what the host (renderer.cpp, rt_host_overlap_volumes) and the device code (rt_overlap.hip) of
// rt_overlap_volumes share: the box-triangle test, the ball acceptance, the node bounds and the walk itself, each as ONE
// inline function both compile, and the launcher's arguments. Built with -ffp-contract=off like everything else, and no
// FMA is written here: f32, every operation rounded once, in the order written; IEEE division and square root. The
// triangle's own box, the outward rounding, the point-triangle distance, the cap and the sorted list are the ones of
// rt_multihit.hpp, rt_lbvh.hpp and rt_closest.hpp, by inclusion.
//
// The answer (include/hrt.h rt_overlap_volumes has the contract in words; DESIGN.md §7h the arguments), per query, with
// rc the root centre, over the tri_geo records (a, e1, e2) in index order:
//   box   (lo, hi). Nothing for a non-finite bound or lo_k > hi_k on an axis. q_lo_k = f32_outward((double)lo_k -
//         (double)rc_k, down), q_hi_k likewise up; c_k = 0.5f lo_k + 0.5f hi_k, h_k = 0.5f hi_k - 0.5f lo_k. Per
//         triangle v0 = a - c first, v1 = v0 + e1, v2 = v0 + e2; the edges f0 = e1, f1 = e2 - e1, f2 = -e2. Triangle j is
//         accepted when
//           1. it has a box box_j (hrt_multihit::tri_box: none for a non-finite a, e1 or e2),
//           2. q_lo_k <= box_j.hi_k && box_j.lo_k <= q_hi_k on all three axes (the comparison the walk makes per node),
//           3. none of the nine axes unit_k x f_i separates: with k1 = (k + 1) % 3, k2 = (k + 2) % 3 the axis has the
//              components a1 = -f_i[k2] at k1 and a2 = f_i[k1] at k2 (no rounding), p_m = a1 v_m[k1] + a2 v_m[k2] per
//              vertex, r = h[k1] |a1| + h[k2] |a2|, and it separates when min(p) > r or max(p) < -r,
//           4. the plane axis n = cross3(e1, e2) does not separate: p_m = (n_x v_m.x + n_y v_m.y) + n_z v_m.z,
//              r = (h_x |n_x| + h_y |n_y|) + h_z |n_z|, the same two comparisons,
//           5. with a cursor, (0.0f, j) lies beyond (after.d2, after.prim): j > after.prim for a cursor that is a record
//              of this query, nothing for the miss record.
//         A comparison that fails (a NaN fails every one) does not separate: touching overlaps, a zero axis never
//         separates, a degenerate triangle answers as the segment or point it is. Records {0.0f, j, 0, 0}, ascending in j.
//   ball  (c, r2), cap = hrt_closest::cap_of(r2). Nothing for a non-finite c or a cap of 0. (d2_j, v, w) =
//         hrt_closest::point_triangle(c, record_j); accepted when d2_j < cap and, with a cursor, (d2_j, j) lies beyond
//         (after.d2, after.prim). Records {d2_j, j, v, w}, ascending in (d2, j).
//   both  the k first accepted in that order, then miss records {RT_T_MISS, -1, 0, 0}; counts: all accepted, not capped.
//
// Why a walk returns exactly that.
//   box   every ancestor's decoded fp16 box contains box_j (pack_child rounds outward at every step), and clause 2 is
//         monotone in the box: a larger box passes wherever a smaller one does. So an accepted triangle's ancestors are all
//         visited, whatever the order; nothing is culled by the list, which sorts by index.
//   ball  the bound is rt_closest.hpp's box_lb2, the function rt_closest.hip's walk culls by, with
//         D = |c - rc| * 1.001 + rr_h and pad = D * 2^-12; for D in [2^-40, 2^60] DESIGN.md §7e ("Culling is exact") gives
//         lb2 < d2_j for every triangle j under the box. A child is visited unless lb2 > bound (equality visits), the bound
//         being the cap, or without counts the d2 of the k-th entry once the list is full: an accepted triangle the final
//         list holds has d2_j <= every bound the walk ever had, so it was visited.
//   flat  a query outside that range, or one that would push a 25th stack word, discards its list and count and runs the
//         flat definition (the loop over all triangles).
#pragma once
#include <stdint.h>

#include "rt_closest.hpp"
#include "rt_lbvh.hpp"
#include "rt_multihit.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HRT_OVERLAP_FN __host__ __device__ inline
#else
#define HRT_OVERLAP_FN inline
#endif

namespace hrt_overlap {

constexpr float T_MISS = 3.40282e+38f;  // RT_T_MISS of include/hrt.h
constexpr uint32_t MAX_K = 16u;         // RT_OVERLAP_MAX_K
constexpr uint32_t KIND_BOX = 1u;       // RT_VOLUME_BOX: 6 floats per query
constexpr uint32_t KIND_BALL = 2u;      // RT_VOLUME_BALL: 4 floats per query
constexpr int STACK = 24;               // entries of the walk's stack (TRI_STACK of rt_kernels.hip)
constexpr uint32_t LEAF_BIT = hrt_lbvh::LEAF_BIT;

struct Hit {  // rt_overlap_hit of include/hrt.h
    float d2;
    int32_t prim;
    float v, w;
};
static_assert(sizeof(Hit) == 16, "rt_overlap_hit: one 16-byte store per record (k_overlap)");

using U4 = hrt_lbvh::U4;
using Tree = hrt_multihit::Tree;    // nodes, order, geo, m, root word, flat, rc, rr_h
using Tally = hrt_multihit::Tally;  // triangle tests, box tests, overflow
using List = hrt_multihit::List;    // the k (key, prim) pairs in ascending order; the box kind's keys are all 0.0f

HRT_OVERLAP_FN uint32_t volume_floats(uint32_t kind) { return kind == KIND_BOX ? 6u : 4u; }
HRT_OVERLAP_FN float fmin3(float a, float b, float c) {
    const float m = b < a ? b : a;
    return c < m ? c : m;
}
HRT_OVERLAP_FN float fmax3(float a, float b, float c) {
    const float m = b > a ? b : a;
    return c > m ? c : m;
}
// The two comparisons of one axis, given the three projections and the box's radius on it. NaN separates nothing.
HRT_OVERLAP_FN bool separates(float p0, float p1, float p2, float r) { return fmin3(p0, p1, p2) > r || fmax3(p0, p1, p2) < -r; }

struct Query {
    // box: the bounds relative to rc, rounded outward; centre and half extent. ball: c, c - rc, the cap and the pad.
    float q_lo[3], q_hi[3], c[3], h[3];
    float cap, pad;
    float after_d2;  // the cursor, when has_after
    int32_t after_j;
    uint32_t has_after;
};

// Clause 2, and the walk's test of a node: closed intervals that share a point on every axis.
HRT_OVERLAP_FN bool boxes_meet(const Query& Q, const float lo[3], const float hi[3]) {
    return Q.q_lo[0] <= hi[0] && lo[0] <= Q.q_hi[0] && Q.q_lo[1] <= hi[1] && lo[1] <= Q.q_hi[1] && Q.q_lo[2] <= hi[2] &&
           lo[2] <= Q.q_hi[2];
}
HRT_OVERLAP_FN bool child_meets(const Query& Q, const U4& ch) {
    const float lo[3] = {hrt_multihit::half_f32(ch.x & 0xFFFFu), hrt_multihit::half_f32(ch.y & 0xFFFFu),
                         hrt_multihit::half_f32(ch.z & 0xFFFFu)};
    const float hi[3] = {hrt_multihit::half_f32(ch.x >> 16), hrt_multihit::half_f32(ch.y >> 16), hrt_multihit::half_f32(ch.z >> 16)};
    return boxes_meet(Q, lo, hi);
}

// False for a box that has no hits by definition.
HRT_OVERLAP_FN bool make_box(const Tree& T, const float b[6], Query& Q) {
    bool good = true;
    for (int k = 0; k < 3; k++) {
        const float lo = b[k], hi = b[3 + k];
        good = good && hrt_lbvh::f32_finite(lo) && hrt_lbvh::f32_finite(hi) && lo <= hi;
        Q.q_lo[k] = hrt_lbvh::f32_outward((double)lo - (double)T.rc[k], false);
        Q.q_hi[k] = hrt_lbvh::f32_outward((double)hi - (double)T.rc[k], true);
        const float hl = 0.5f * lo, hh = 0.5f * hi;
        Q.c[k] = hl + hh;
        Q.h[k] = hh - hl;
    }
    Q.cap = 0.0f;
    Q.pad = 0.0f;
    return good;
}
// False for a ball that has no hits by definition; covered: the walk's bound holds for it. q_lo holds c - rc.
HRT_OVERLAP_FN bool make_ball(const Tree& T, const float b[4], Query& Q, bool& covered) {
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        Q.c[k] = b[k];
        Q.q_lo[k] = b[k] - T.rc[k];
        Q.q_hi[k] = 0.0f;
        Q.h[k] = 0.0f;
        finite = finite && hrt_lbvh::f32_finite(b[k]);
    }
    Q.cap = hrt_closest::cap_of(b[3]);
    const float D = __builtin_sqrtf(hrt_closest::dot3(Q.q_lo, Q.q_lo)) * 1.001f + T.rr_h;
    covered = D >= hrt_closest::D_MIN && D <= hrt_closest::D_MAX;
    Q.pad = D * hrt_closest::PAD;
    return finite && Q.cap > 0.0f;
}

// Clauses 1 to 4 of the box kind.
HRT_OVERLAP_FN bool box_triangle(const Query& Q, const Tree& T, const float g[9]) {
    float lo[3], hi[3];
    if (!hrt_multihit::tri_box(g, T.rc, lo, hi)) return false;
    if (!boxes_meet(Q, lo, hi)) return false;
    float v0[3], v1[3], v2[3], f[3][3];
    for (int k = 0; k < 3; k++) {
        v0[k] = g[k] - Q.c[k];
        v1[k] = v0[k] + g[3 + k];
        v2[k] = v0[k] + g[6 + k];
        f[0][k] = g[3 + k];
        f[1][k] = g[6 + k] - g[3 + k];
        f[2][k] = -g[6 + k];
    }
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int i = 0; i < 3; i++) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
        for (int k = 0; k < 3; k++) {
            const int k1 = (k + 1) % 3, k2 = (k + 2) % 3;
            const float a1 = -f[i][k2], a2 = f[i][k1];
            const float x0 = a1 * v0[k1], y0 = a2 * v0[k2], x1 = a1 * v1[k1], y1 = a2 * v1[k2], x2 = a1 * v2[k1],
                        y2 = a2 * v2[k2];
            const float rx = Q.h[k1] * __builtin_fabsf(a1), ry = Q.h[k2] * __builtin_fabsf(a2);
            if (separates(x0 + y0, x1 + y1, x2 + y2, rx + ry)) return false;
        }
    }
    float n[3];
    hrt_multihit::cross3(g + 3, g + 6, n);
    const float p0 = hrt_closest::dot3(n, v0), p1 = hrt_closest::dot3(n, v1), p2 = hrt_closest::dot3(n, v2);
    const float an[3] = {__builtin_fabsf(n[0]), __builtin_fabsf(n[1]), __builtin_fabsf(n[2])};
    return !separates(p0, p1, p2, hrt_closest::dot3(Q.h, an));
}

// Triangle j against the list and the count.
template <uint32_t KIND>
HRT_OVERLAP_FN void test_triangle(const Query& Q, const Tree& T, uint32_t j, List& L, uint32_t& count) {
    const float* const g = T.geo + 9 * (size_t)j;
    float key = 0.0f;
    if (KIND == KIND_BOX) {
        if (!box_triangle(Q, T, g)) return;
    } else {
        key = hrt_closest::point_triangle(Q.c, g).d2;
        if (!(key < Q.cap)) return;
    }
    if (Q.has_after != 0u && !hrt_multihit::hit_less(Q.after_d2, Q.after_j, key, (int32_t)j)) return;
    count += 1u;
    if (hrt_multihit::list_takes(L, key, (int32_t)j)) hrt_multihit::list_insert(L, key, (int32_t)j);
}

// The flat definition: every triangle in index order.
template <uint32_t KIND>
HRT_OVERLAP_FN void flat(const Query& Q, const Tree& T, List& L, uint32_t& count) {
    L.n = 0u;
    count = 0u;
    for (uint32_t j = 0; j < T.m; j++) test_triangle<KIND>(Q, T, j, L, count);
}

// One query. vol: the query's 6 or 4 floats. stack: STACK words at `sstride`. The list's storage is the caller's (L.lt,
// L.lj, L.stride, L.k); on return L.n entries are valid and `count` is the number of accepted triangles (COUNT_ALL; else
// it counts what the walk met and nobody reads it). Box: the left child first, the right one pushed. Ball: the nearer
// child first; a child is visited unless lb2 > bound.
template <uint32_t KIND, bool COUNT_ALL, bool STATS>
HRT_OVERLAP_FN void query(const Tree& T, const float* vol, bool has_after, float after_d2, int32_t after_j, uint32_t* stack,
                          uint32_t sstride, List& L, uint32_t& count, Tally& tally) {
    L.n = 0u;
    count = 0u;
    Query Q;
    bool covered = true;
    if (!(KIND == KIND_BOX ? make_box(T, vol, Q) : make_ball(T, vol, Q, covered))) return;
    Q.has_after = has_after ? 1u : 0u;
    Q.after_d2 = after_d2;
    Q.after_j = after_j;
    if (T.flat != 0u || !covered) {
        flat<KIND>(Q, T, L, count);
        if (STATS) tally.tri += T.m;
        return;
    }
    uint32_t node = T.root;
    int sp = 0;
    float bound = Q.cap;
    while (true) {
        if ((node & LEAF_BIT) == 0u) {
            const U4 lc = T.hnodes[2 * (size_t)node], rc = T.hnodes[2 * (size_t)node + 1];
            bool hl, hr, lfirst = true;
            if (KIND == KIND_BOX) {
                hl = child_meets(Q, lc);
                hr = child_meets(Q, rc);
            } else {
                const float ll = hrt_closest::box_lb2(lc, Q.q_lo, Q.pad), lr = hrt_closest::box_lb2(rc, Q.q_lo, Q.pad);
                hl = !(ll > bound);
                hr = !(lr > bound);
                lfirst = ll <= lr;
            }
            if (STATS) tally.box += 2u;
            if (hl && hr) {
                if (sp == STACK) {
                    tally.overflow = 1u;
                    flat<KIND>(Q, T, L, count);
                    if (STATS) tally.tri += T.m;
                    return;
                }
                stack[(uint32_t)sp * sstride] = lfirst ? rc.w : lc.w;
                sp++;
                node = lfirst ? lc.w : rc.w;
                continue;
            }
            if (hl) { node = lc.w; continue; }
            if (hr) { node = rc.w; continue; }
        } else {
            const uint32_t first = (node >> 4) & 0x07FFFFFFu, cnt = node & 15u;
            for (uint32_t s = 0; s < cnt; s++) test_triangle<KIND>(Q, T, T.order[first + s], L, count);
            if (STATS) tally.tri += cnt;
            if (KIND == KIND_BALL && !COUNT_ALL && L.k != 0u && L.n == L.k) bound = L.lt[(L.k - 1u) * L.stride];
        }
        if (sp == 0) break;
        node = stack[(uint32_t)(--sp) * sstride];
    }
}

// Record s of a finished query: the list's entry (the ball kind with point_triangle's own v, w, recomputed: the walk keeps
// d2 and prim only), or the miss record.
template <uint32_t KIND>
HRT_OVERLAP_FN Hit make_record(const Tree& T, const float* vol, const List& L, uint32_t s) {
    Hit h{T_MISS, -1, 0.0f, 0.0f};
    if (s >= L.n) return h;
    h.prim = L.lj[s * L.stride];
    h.d2 = L.lt[s * L.stride];
    if (KIND == KIND_BALL) {
        const hrt_closest::Nearest c = hrt_closest::point_triangle(vol, T.geo + 9 * (size_t)h.prim);
        h.v = c.v;
        h.w = c.w;
    }
    return h;
}

// ---- the launcher's arguments (rt_overlap.hip) ----
struct Launch {
    Tree tree;
    const float* volumes;  // 6 n or 4 n floats
    const Hit* after;      // n records or null
    void* hits;            // n k records
    uint32_t* counts;      // n words or null
    uint32_t n, k, kind;
    unsigned long long* stats;  // the counting instantiation's four words (include/hrt_testing.h); else unused
};

// ---- the host mirror ----
// n queries: the walk on T, or the flat definition for T.flat. hits: n k records; counts: n words or null (the ball walk
// then culls by the list, as the device does).
template <uint32_t KIND>
inline void host_overlap_kind(const Tree& T, const float* volumes, const Hit* after, uint32_t n, uint32_t k, Hit* hits,
                              uint32_t* counts) {
    uint32_t stack[STACK];
    float lt[MAX_K];
    int32_t lj[MAX_K];
    const uint32_t w = volume_floats(KIND);
    for (uint32_t i = 0; i < n; i++) {
        const float* const vol = volumes + w * (size_t)i;
        List L{lt, lj, 1u, k, 0u};
        uint32_t count = 0u;
        Tally tally{0u, 0u, 0u};
        const bool cur = after != nullptr;
        const float ad = cur ? after[i].d2 : 0.0f;
        const int32_t aj = cur ? after[i].prim : -1;
        if (counts) query<KIND, true, false>(T, vol, cur, ad, aj, stack, 1u, L, count, tally);
        else query<KIND, false, false>(T, vol, cur, ad, aj, stack, 1u, L, count, tally);
        for (uint32_t s = 0; s < k; s++) hits[(size_t)i * k + s] = make_record<KIND>(T, vol, L, s);
        if (counts) counts[i] = count;
    }
}
inline void host_overlap(const Tree& T, uint32_t kind, const float* volumes, const Hit* after, uint32_t n, uint32_t k, Hit* hits,
                         uint32_t* counts) {
    if (kind == KIND_BOX) host_overlap_kind<KIND_BOX>(T, volumes, after, n, k, hits, counts);
    else host_overlap_kind<KIND_BALL>(T, volumes, after, n, k, hits, counts);
}

}  // namespace hrt_overlap
