// rt_closest.hpp — what the host (renderer.cpp, rt_host_closest_points) and the device code (rt_closest.hip) of
// rt_closest_points share: the point-triangle distance as ONE inline function both compile, the acceptance rule, the
// definition of the query as a loop over every triangle (host_closest, the mirror the tests compare the device with, bit
// for bit), and the launcher's arguments. Built with -ffp-contract=off like everything else, and no FMA is written here:
// f32 only, every operation rounded once, in the order written; IEEE division.
//
// The function (include/hrt.h rt_closest_points has the contract in words; DESIGN.md §7e the arguments):
//   input      the point p and a triangle's tri_geo record (a, e1, e2: 9 floats; e1 = b - a, e2 = c - a in f32).
//   ap         p - a first, so a mesh far from the origin loses nothing: everything after it is relative to a.
//   candidates the nearest point of each edge as a clamped segment parameter — ab (v = t, w = 0), ac (v = 0, w = t),
//              bc (w = s, v = 1 - s rounded down) — and the plane projection (v, w) by Cramer's rule, as solved and again
//              after one step of refinement, each when it passes v >= 0, w >= 0, fl(v + w) < 1. A zero denominator (a
//              zero-length edge, a zero-area triangle) is a branch: the parameter is 0, the projection is not tried.
//   d2         of a candidate: |ap - (v e1 + w e2)|^2 of exactly its v, w (dist2). The answer is the candidate with the
//              smallest d2, the earlier one of equal d2, in the order ab, ac, bc, plane, refined plane.
//   hull       v >= 0, w >= 0, v + w <= 1 as real numbers, for every input (clamps; bc_weights; the strict test of the
//              projection): the point a + v e1 + w e2 lies in the triangle's hull, which the tree's boxes contain.
//   non-finite a non-finite p, a, e1 or e2 gives d2 = NaN (v = w = 0), which accept() never takes. Finite input never
//              gives NaN: an overflow makes d2 +inf, which no cap admits either (every cap is at most RT_T_MISS).
#pragma once
#include <stdint.h>

#include "rt_lbvh.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HRT_CLOSEST_FN __host__ __device__ inline
#else
#define HRT_CLOSEST_FN inline
#endif

namespace hrt_closest {

constexpr float T_MISS = 3.40282e+38f;  // RT_T_MISS of include/hrt.h

struct Record {  // rt_closest of include/hrt.h
    float d2;
    int32_t prim;
    float p[3];
    float v, w;
    uint32_t reserved;
};
static_assert(sizeof(Record) == 32, "rt_closest: two 16-byte stores per record (k_closest_points)");

struct Nearest {
    float d2, v, w;
};

using hrt_lbvh::f32_finite;
using hrt_lbvh::quiet_nan;
using U4 = hrt_lbvh::U4;  // half a node: one child's six halves and its word (rt_lbvh.hpp pack_child)
constexpr uint32_t LEAF_BIT = hrt_lbvh::LEAF_BIT;
HRT_CLOSEST_FN float dot3(const float a[3], const float b[3]) {
    const float x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    return (x + y) + z;
}
// [0, 1], +0 for NaN, -0 and everything below 0.
HRT_CLOSEST_FN float clamp01(float t) { return !(t > 0.0f) ? 0.0f : (t > 1.0f ? 1.0f : t); }
// The parameter of the nearest point of the segment o + t e, t in [0, 1]: xe = (p - o) . e, ee = e . e.
HRT_CLOSEST_FN float segment_t(float xe, float ee) { return ee > 0.0f ? clamp01(xe / ee) : 0.0f; }
// |ap - (v e1 + w e2)|^2 (g: a, e1, e2).
HRT_CLOSEST_FN float dist2(const float ap[3], const float g[9], float v, float w) {
    float r[3];
    for (int k = 0; k < 3; k++) {
        const float ve = v * g[3 + k], we = w * g[6 + k];
        r[k] = ap[k] - (ve + we);
    }
    return dot3(r, r);
}
// The weights of the point b + s (c - b), s in [0, 1]: w = s and the largest f32 v with v + s <= 1. 1 - s is exact for
// s >= 0.5; below that it can round up by at most half an ulp of [0.5, 1], which 1 - v (exact there) shows.
HRT_CLOSEST_FN float bc_weight_v(float s) {
    float v = 1.0f - s;
    if (1.0f - v < s) v = v - 0x1p-24f;
    return v;
}

// One unknown of [d11 d12; d12 d22] (v, w) = (b1, b2) by Cramer's rule: v = (d22 b1 - d12 b2) / det; w is the same with
// the roles swapped (b2, b1, d12, d11).
HRT_CLOSEST_FN float solve_v(float b1, float b2, float d12, float d22, float det) {
    const float x = d22 * b1, y = d12 * b2;
    return (x - y) / det;
}
// A point of the plane as a candidate: only with v >= 0, w >= 0 and fl(v + w) < 1, which implies v + w < 1 (rounding is
// monotonic, and 1 is a float). NaN fails the tests.
HRT_CLOSEST_FN void inside_candidate(const float ap[3], const float g[9], float v, float w, Nearest& best) {
    v = v + 0.0f;  // (-0 -> +0)
    w = w + 0.0f;
    if (v >= 0.0f && w >= 0.0f && v + w < 1.0f) {
        const float d = dist2(ap, g, v, w);
        if (d < best.d2) best = Nearest{d, v, w};
    }
}

HRT_CLOSEST_FN Nearest point_triangle(const float p[3], const float g[9]) {
    bool finite = f32_finite(p[0]) && f32_finite(p[1]) && f32_finite(p[2]);
    for (int k = 0; k < 9; k++) finite = finite && f32_finite(g[k]);
    const float* e1 = g + 3;
    const float* e2 = g + 6;
    const float ap[3] = {p[0] - g[0], p[1] - g[1], p[2] - g[2]};
    const float d1 = dot3(ap, e1), d2 = dot3(ap, e2);
    const float d11 = dot3(e1, e1), d12 = dot3(e1, e2), d22 = dot3(e2, e2);
    // ab
    Nearest best;
    best.v = segment_t(d1, d11);
    best.w = 0.0f;
    best.d2 = dist2(ap, g, best.v, best.w);
    // ac
    {
        const float w = segment_t(d2, d22);
        const float d = dist2(ap, g, 0.0f, w);
        if (d < best.d2) best = Nearest{d, 0.0f, w};
    }
    // bc
    {
        const float e3[3] = {e2[0] - e1[0], e2[1] - e1[1], e2[2] - e1[2]};
        const float bp[3] = {ap[0] - e1[0], ap[1] - e1[1], ap[2] - e1[2]};
        const float s = segment_t(dot3(bp, e3), dot3(e3, e3));
        const float v = bc_weight_v(s);
        const float d = dist2(ap, g, v, s);
        if (d < best.d2) best = Nearest{d, v, s};
    }
    // the plane projection by Cramer's rule, then the same after one step of refinement on its residual (the residual is
    // small near the surface, so the second solve loses little where the first one, on a thin triangle, loses most)
    const float m1 = d11 * d22, m2 = d12 * d12;
    const float det = m1 - m2;
    if (det > 0.0f) {
        const float v0 = solve_v(d1, d2, d12, d22, det), w0 = solve_v(d2, d1, d12, d11, det);
        inside_candidate(ap, g, v0, w0, best);
        float r[3];
        for (int k = 0; k < 3; k++) {
            const float ve = v0 * e1[k], we = w0 * e2[k];
            r[k] = ap[k] - (ve + we);
        }
        const float g1 = dot3(r, e1), g2 = dot3(r, e2);
        const float dv = solve_v(g1, g2, d12, d22, det), dw = solve_v(g2, g1, d12, d11, det);
        inside_candidate(ap, g, v0 + dv, w0 + dw, best);
    }
    if (!finite) best = Nearest{quiet_nan(), 0.0f, 0.0f};
    return best;
}

// The cap of query i: 0 for "nothing can be accepted" (NaN, -0, everything <= 0), else min(maxd2, RT_T_MISS).
HRT_CLOSEST_FN float cap_of(float maxd2) { return !(maxd2 > 0.0f) ? 0.0f : (maxd2 < T_MISS ? maxd2 : T_MISS); }
// The lexicographic minimum of (d2, j) below the cap: best starts at the cap with bj = -1. NaN is never accepted.
HRT_CLOSEST_FN bool accept(float d2, int32_t j, float best, int32_t bj) {
    return d2 < best || (d2 == best && bj >= 0 && j < bj);
}
// Triangle j against the running answer (best, bj, bv, bw).
HRT_CLOSEST_FN void test_triangle(const float p[3], const float* geo, uint32_t j, float& best, int32_t& bj, float& bv,
                                  float& bw) {
    const Nearest c = point_triangle(p, geo + 9 * (size_t)j);
    if (accept(c.d2, (int32_t)j, best, bj)) {
        best = c.d2;
        bj = (int32_t)j;
        bv = c.v;
        bw = c.w;
    }
}
HRT_CLOSEST_FN Record make_record(const float* geo, float best, int32_t bj, float bv, float bw) {
    Record r{T_MISS, -1, {0.0f, 0.0f, 0.0f}, 0.0f, 0.0f, 0u};
    if (bj < 0) return r;
    const float* g = geo + 9 * (size_t)bj;
    r.d2 = best;
    r.prim = bj;
    for (int k = 0; k < 3; k++) {
        const float ve = bv * g[3 + k], we = bw * g[6 + k];
        r.p[k] = g[k] + (ve + we);
    }
    r.v = bv;
    r.w = bw;
    return r;
}

// The definition: every triangle, in index order. geo: 9 m floats; maxd2: n floats or null; out: n records.
inline void host_closest(const float* geo, uint32_t m, const float* points, const float* maxd2, uint32_t n, Record* out) {
    for (uint32_t i = 0; i < n; i++) {
        const float* p = points + 3 * (size_t)i;
        float best = cap_of(maxd2 ? maxd2[i] : T_MISS), bv = 0.0f, bw = 0.0f;
        int32_t bj = -1;
        if (best > 0.0f)
            for (uint32_t j = 0; j < m; j++) test_triangle(p, geo, j, best, bj, bv, bw);
        out[i] = make_record(geo, best, bj, bv, bw);
    }
}

// ---- the walk's bound (rt_closest.hip; DESIGN.md §7e "Culling is exact") ----
// D = |p - rc| * 1.001 + rr_h bounds every length the function and the bound handle; the walk runs for D in
// [D_MIN, D_MAX] (no product of two such lengths overflows, and no underflow reaches the pad), pad = D * PAD.
constexpr float D_MIN = 0x1p-40f, D_MAX = 0x1p60f, PAD = 0x1p-12f;
constexpr int STACK = 24;  // entries of the walk's stack (TRI_STACK of rt_kernels.hip)

// One axis of the bound: how far q lies outside [lo, hi] (the two halves of w), less the pad, not below 0. (lo is never
// +inf, hi never -inf, q is finite: no NaN; an infinite half on the far side gives -inf, which the max drops.)
HRT_CLOSEST_FN float axis_gap(uint32_t w, float q, float pad) {
    const float below = (float)hrt_lbvh::f16_from_bits((uint16_t)(w & 0xFFFFu)) - q;
    const float above = q - (float)hrt_lbvh::f16_from_bits((uint16_t)(w >> 16));
    const float g = (below > above ? below : above) - pad;
    return g > 0.0f ? g : 0.0f;
}
// The lower bound of the squared distance from q (relative to the root centre) to a child's box, taken pad closer: the
// one definition rt_closest.hip's walk and rt_overlap.hpp's ball walk both cull by.
HRT_CLOSEST_FN float box_lb2(const U4& c, const float q[3], float pad) {
    const float gx = axis_gap(c.x, q[0], pad), gy = axis_gap(c.y, q[1], pad), gz = axis_gap(c.z, q[2], pad);
    return (gx * gx + gy * gy) + gz * gz;
}

struct Launch {
    const U4* hnodes;       // the node array: two U4 per node (rt_lbvh.hpp pack_child)
    const uint32_t* order;  // tb_order: the triangle index of every leaf position
    const float* geo;       // tri_geo: 9 m floats
    uint32_t m, root;       // triangles in geo; the root word
    float rc[3], rr_h;      // root centre; the radius bound of the fp16 boxes
    const float* points;    // 3 n floats
    const float* maxd2;     // n floats or null
    void* out;              // n Records
    uint32_t n;
    unsigned long long* counts;  // the counting instantiation's four words (include/hrt_testing.h); else unused
};

}  // namespace hrt_closest
