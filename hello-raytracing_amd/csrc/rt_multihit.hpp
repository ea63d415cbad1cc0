// rt_multihit.hpp — what the host (renderer.cpp, rt_host_cast_rays_multi) and the device code (rt_multihit.hip) of
// rt_cast_rays_multi share: the query constants, the slab test, a triangle's own box, the triangle test, the sorted
// insertion and the walk itself, each as ONE inline function both compile, and the launcher's arguments. Built with
// -ffp-contract=off like everything else: f32, every operation rounded once, in the order written; IEEE division and square
// root; an FMA only where __builtin_fmaf is written (the slab planes, and the three dots of the triangle test, which are
// rt_device.hpp's `dot`).
//
// The answer (include/hrt.h rt_cast_rays_multi has the contract in words; DESIGN.md §7g the arguments). Per ray, with rc and
// rr_h the root centre and the radius bound of the fp16 boxes:
//   constants  op = o - rc, D = sqrt(op . op) * 1.001 + rr_h, pad = D * 2^-12, inv_k = |d_k| >= 1e-30 ? 1 / d_k :
//              copysign(1e30, d_k), c_lo_k = (-op_k - pad) * inv_k, c_hi_k = (-op_k + pad) * inv_k (make_query).
//   slab       of a box [lo, hi] relative to rc under `upper`: per axis t0 = fma(lo, inv, c_lo), t1 = fma(hi, inv, c_hi);
//              enter = max(min(t0, t1) over the axes, 0), exit = min(max(t0, t1) over the axes, upper); hit when
//              enter <= exit. Minimum and maximum are comparisons and selects (slab).
//   box_j      rt_lbvh.hpp's tri_bounds f64 box of triangle j through f32_outward, each bound then
//              (float)((double)v - (double)rc_k) (tri_box). A triangle with a non-finite a, e1 or e2 has no box.
//   accepted   triangle j is, when it has a box, tri_test accepts it (rt_kernels.hip's tri_t restated: the same
//              operations in the same order, 1 / det the IEEE division), 1e-4 <= t_j < cap, (t_j, j) lies beyond the
//              cursor when one is given, and slab(box_j, t_j) is hit (accepted()).
//   records    the k smallest accepted (t_j, j), ascending; counts: the number of all accepted triangles.
//   nothing    for a ray with a non-finite component of o or d or a non-finite D, and for cap = 0.
//
// Why a walk that culls by enter > bound returns exactly that: every ancestor's decoded fp16 box contains box_j, the
// slab is monotone in the box (an FMA rounds monotonically, and inv, c_lo, c_hi do not depend on the box), so
// slab(box_j, t_j) hit implies every ancestor's slab is hit under every bound >= t_j.
#pragma once
#include <stdint.h>

#include "rt_lbvh.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HRT_MULTIHIT_FN __host__ __device__ inline
#else
#define HRT_MULTIHIT_FN inline
#endif

namespace hrt_multihit {

constexpr float T_MISS = 3.40282e+38f;  // RT_T_MISS of include/hrt.h
constexpr uint32_t MAX_K = 16u;         // RT_MULTI_HIT_MAX_K
constexpr int STACK = 24;               // entries of the walk's stack (TRI_STACK of rt_kernels.hip)
constexpr uint32_t LEAF_BIT = hrt_lbvh::LEAF_BIT;

struct Hit {  // rt_multi_hit of include/hrt.h
    float t;
    int32_t prim;
    float u, v;
};
static_assert(sizeof(Hit) == 16, "rt_multi_hit: one 16-byte store per record (k_cast_rays_multi)");

using U4 = hrt_lbvh::U4;

struct Tree {
    const U4* hnodes;       // two U4 per node slot (rt_lbvh.hpp pack_child)
    const uint32_t* order;  // the triangle index of every leaf position
    const float* geo;       // tri_geo: 9 m floats (a, e1, e2)
    uint32_t m, root;       // triangles in geo; the root word
    uint32_t flat;          // 1: no nodes are given, every query runs the flat definition
    float rc[3], rr_h;      // root centre; the radius bound of the fp16 boxes
};
struct Tally {
    uint32_t tri, box, overflow;
};

HRT_MULTIHIT_FN bool f32_finite(float x) { return hrt_lbvh::f32_finite(x); }
// rt_device.hpp's dot: the x product, then one FMA per further axis.
HRT_MULTIHIT_FN float dot3(const float a[3], const float b[3]) {
    return __builtin_fmaf(a[2], b[2], __builtin_fmaf(a[1], b[1], a[0] * b[0]));
}
HRT_MULTIHIT_FN void cross3(const float a[3], const float b[3], float out[3]) {
    out[0] = a[1] * b[2] - a[2] * b[1];
    out[1] = a[2] * b[0] - a[0] * b[2];
    out[2] = a[0] * b[1] - a[1] * b[0];
}
HRT_MULTIHIT_FN float half_f32(uint32_t bits16) { return (float)hrt_lbvh::f16_from_bits((uint16_t)bits16); }

// The cap of a ray (rt_occluded's tmax rules): 0 for "nothing can be accepted" (NaN, -0, everything <= 0), else
// min(tmax, RT_T_MISS).
HRT_MULTIHIT_FN float cap_of(float tmax) { return !(tmax > 0.0f) ? 0.0f : (tmax < T_MISS ? tmax : T_MISS); }

struct Query {
    float o[3], d[3];
    float inv[3], c_lo[3], c_hi[3];
    float cap;        // 0: nothing is accepted
    float after_t;    // the cursor, when has_after
    int32_t after_j;
    uint32_t has_after;
};

// False for a ray that has no hits by definition (non-finite o, d or D); Q.cap = 0 likewise accepts nothing.
// The cursor is given by value (has_after, after_t, after_j).
HRT_MULTIHIT_FN bool make_query(const Tree& T, const float o[3], const float d[3], float tmax, bool has_after, float after_t,
                                int32_t after_j, Query& Q) {
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        Q.o[k] = o[k];
        Q.d[k] = d[k];
        finite = finite && f32_finite(o[k]) && f32_finite(d[k]);
    }
    Q.cap = cap_of(tmax);
    Q.has_after = has_after ? 1u : 0u;
    Q.after_t = after_t;
    Q.after_j = after_j;
    const float op[3] = {o[0] - T.rc[0], o[1] - T.rc[1], o[2] - T.rc[2]};
    const float xx = op[0] * op[0], yy = op[1] * op[1], zz = op[2] * op[2];
    const float D = __builtin_sqrtf((xx + yy) + zz) * 1.001f + T.rr_h;
    const float pad = D * 0x1p-12f;
    for (int k = 0; k < 3; k++) {
        Q.inv[k] = __builtin_fabsf(d[k]) >= 1e-30f ? 1.0f / d[k] : __builtin_copysignf(1e30f, d[k]);
        Q.c_lo[k] = (-op[k] - pad) * Q.inv[k];
        Q.c_hi[k] = (-op[k] + pad) * Q.inv[k];
    }
    return finite && f32_finite(D);
}

// The slab of the box [lo, hi] (relative to rc) under `upper`; enter: where the ray enters it, not below 0.
HRT_MULTIHIT_FN bool slab(const Query& Q, const float lo[3], const float hi[3], float upper, float& enter) {
    float e = 0.0f, x = upper;
    for (int k = 0; k < 3; k++) {
        const float t0 = __builtin_fmaf(lo[k], Q.inv[k], Q.c_lo[k]), t1 = __builtin_fmaf(hi[k], Q.inv[k], Q.c_hi[k]);
        const float mn = t1 < t0 ? t1 : t0, mx = t1 > t0 ? t1 : t0;
        e = mn > e ? mn : e;
        x = mx < x ? mx : x;
    }
    enter = e;
    return e <= x;
}
// One child of a node: its six halves decoded (half to float is exact).
HRT_MULTIHIT_FN bool slab_child(const Query& Q, const U4& c, float upper, float& enter) {
    const float lo[3] = {half_f32(c.x & 0xFFFFu), half_f32(c.y & 0xFFFFu), half_f32(c.z & 0xFFFFu)};
    const float hi[3] = {half_f32(c.x >> 16), half_f32(c.y >> 16), half_f32(c.z >> 16)};
    return slab(Q, lo, hi, upper, enter);
}

// Triangle j's own box relative to rc. False: a non-finite triangle, which has none.
HRT_MULTIHIT_FN bool tri_box(const float aee[9], const float rc[3], float lo[3], float hi[3]) {
    double dlo[3], dhi[3], cen[3];
    if (!hrt_lbvh::tri_bounds(aee, dlo, dhi, cen)) return false;
    for (int k = 0; k < 3; k++) {
        lo[k] = (float)((double)hrt_lbvh::f32_outward(dlo[k], false) - (double)rc[k]);
        hi[k] = (float)((double)hrt_lbvh::f32_outward(dhi[k], true) - (double)rc[k]);
    }
    return true;
}

// tri_t of rt_kernels.hip (Moller-Trumbore), with u and v kept. False when the determinant, u or v test rejects.
HRT_MULTIHIT_FN bool tri_test(const float o[3], const float d[3], const float aee[9], float& t, float& u, float& v) {
    const float* const e1 = aee + 3;
    const float* const e2 = aee + 6;
    float hh[3], q[3];
    cross3(d, e2, hh);
    const float det = dot3(e1, hh);
    if (__builtin_fabsf(det) < 1e-4f) return false;
    const float inv_det = 1.0f / det;
    const float s[3] = {o[0] - aee[0], o[1] - aee[1], o[2] - aee[2]};
    u = inv_det * dot3(s, hh);
    if (u < 0.0f || u > 1.0f) return false;
    cross3(s, e1, q);
    v = inv_det * dot3(d, q);
    if (v < 0.0f || u + v > 1.0f) return false;
    t = inv_det * dot3(e2, q);
    return true;
}

// (t, j) < (bt, bj), lexicographically.
HRT_MULTIHIT_FN bool hit_less(float t, int32_t j, float bt, int32_t bj) { return t < bt || (t == bt && j < bj); }

// Everything of the acceptance but the slab clause: the triangle test, the range and the cursor.
HRT_MULTIHIT_FN bool candidate(const Query& Q, const float aee[9], int32_t j, float& t) {
    float u, v;
    if (!tri_test(Q.o, Q.d, aee, t, u, v)) return false;
    if (!(t >= 1e-4f && t < Q.cap)) return false;
    if (Q.has_after != 0u && !hit_less(Q.after_t, Q.after_j, t, j)) return false;
    return true;
}
// The slab clause: the computed t does not lie before the ray enters its own triangle's padded box.
HRT_MULTIHIT_FN bool own_box_hit(const Query& Q, const Tree& T, const float aee[9], float t) {
    float lo[3], hi[3], enter;
    if (!tri_box(aee, T.rc, lo, hi)) return false;
    return slab(Q, lo, hi, t, enter);
}
HRT_MULTIHIT_FN bool accepted(const Query& Q, const Tree& T, uint32_t j, float& t) {
    const float* const aee = T.geo + 9 * (size_t)j;
    return candidate(Q, aee, (int32_t)j, t) && own_box_hit(Q, T, aee, t);
}

// The per-query list: up to k (t, prim) pairs in ascending order, entry s at lt[s * stride], lj[s * stride].
struct List {
    float* lt;
    int32_t* lj;
    uint32_t stride, k, n;
};
HRT_MULTIHIT_FN bool list_takes(const List& L, float t, int32_t j) {
    if (L.n < L.k) return true;
    return L.k != 0u && hit_less(t, j, L.lt[(L.k - 1u) * L.stride], L.lj[(L.k - 1u) * L.stride]);
}
// (t, j), which list_takes accepted, at its place; a full list drops its last entry.
HRT_MULTIHIT_FN void list_insert(List& L, float t, int32_t j) {
    uint32_t pos = L.n < L.k ? L.n++ : L.k - 1u;
    while (pos > 0u && hit_less(t, j, L.lt[(pos - 1u) * L.stride], L.lj[(pos - 1u) * L.stride])) {
        L.lt[pos * L.stride] = L.lt[(pos - 1u) * L.stride];
        L.lj[pos * L.stride] = L.lj[(pos - 1u) * L.stride];
        pos--;
    }
    L.lt[pos * L.stride] = t;
    L.lj[pos * L.stride] = j;
}

// Triangle j against the list and the count. COUNT_ALL: every accepted triangle is counted, so the slab clause is
// evaluated for every candidate; else only for one the list would take (the records are the same).
template <bool COUNT_ALL>
HRT_MULTIHIT_FN void test_triangle(const Query& Q, const Tree& T, uint32_t j, List& L, uint32_t& count) {
    const float* const aee = T.geo + 9 * (size_t)j;
    float t;
    if (!candidate(Q, aee, (int32_t)j, t)) return;
    const bool takes = list_takes(L, t, (int32_t)j);
    if (!COUNT_ALL && !takes) return;
    if (!own_box_hit(Q, T, aee, t)) return;
    count += 1u;
    if (takes) list_insert(L, t, (int32_t)j);
}

// The flat definition: every triangle in index order.
template <bool COUNT_ALL>
HRT_MULTIHIT_FN void flat(const Query& Q, const Tree& T, List& L, uint32_t& count) {
    L.n = 0u;
    count = 0u;
    for (uint32_t j = 0; j < T.m; j++) test_triangle<COUNT_ALL>(Q, T, j, L, count);
}

// One query. stack: STACK words at `sstride`. The list's storage is the caller's (L.lt, L.lj, L.stride, L.k); on return
// L.n entries are valid and `count` is the number of accepted triangles (COUNT_ALL; else it counts what was evaluated
// and nobody reads it). The walk visits a child unless enter > bound (equality visits), the nearer one first; the bound is
// the cap, or with !COUNT_ALL the t of the k-th entry once the list is full. A query that would need a word past the
// stack discards list and count and runs the flat definition.
template <bool COUNT_ALL, bool STATS>
HRT_MULTIHIT_FN void query(const Tree& T, const float o[3], const float d[3], float tmax, bool has_after, float after_t,
                           int32_t after_j, uint32_t* stack, uint32_t sstride, List& L, uint32_t& count, Tally& tally) {
    L.n = 0u;
    count = 0u;
    Query Q;
    if (!make_query(T, o, d, tmax, has_after, after_t, after_j, Q) || !(Q.cap > 0.0f)) return;
    if (T.flat != 0u) {
        flat<COUNT_ALL>(Q, T, L, count);
        if (STATS) tally.tri += T.m;
        return;
    }
    uint32_t node = T.root;
    int sp = 0;
    float bound = Q.cap;
    while (true) {
        if ((node & LEAF_BIT) == 0u) {
            const U4 lc = T.hnodes[2 * (size_t)node], rc = T.hnodes[2 * (size_t)node + 1];
            float tl, tr;
            const bool hl = slab_child(Q, lc, bound, tl), hr = slab_child(Q, rc, bound, tr);
            if (STATS) tally.box += 2u;
            if (hl && hr) {
                const bool lfirst = tl <= tr;
                if (sp == STACK) {
                    tally.overflow = 1u;
                    flat<COUNT_ALL>(Q, T, L, count);
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
            for (uint32_t s = 0; s < cnt; s++) test_triangle<COUNT_ALL>(Q, T, T.order[first + s], L, count);
            if (STATS) tally.tri += cnt;
            if (!COUNT_ALL && L.k != 0u && L.n == L.k) bound = L.lt[(L.k - 1u) * L.stride];
        }
        if (sp == 0) break;
        node = stack[(uint32_t)(--sp) * sstride];
    }
}

// Record s of a finished query: the list's entry with the test's own u, v (recomputed: the walk keeps t and prim only),
// or the miss record.
HRT_MULTIHIT_FN Hit make_record(const Tree& T, const float o[3], const float d[3], const List& L, uint32_t s) {
    Hit h{T_MISS, -1, 0.0f, 0.0f};
    if (s >= L.n) return h;
    h.prim = L.lj[s * L.stride];
    float t;
    tri_test(o, d, T.geo + 9 * (size_t)h.prim, t, h.u, h.v);
    h.t = L.lt[s * L.stride];
    return h;
}

// ---- the launcher's arguments (rt_multihit.hip) ----
struct Launch {
    Tree tree;
    const float* origins;  // 3 n floats
    const float* dirs;     // 3 n floats
    const float* tmax;     // n floats or null
    const Hit* after;      // n records or null
    void* hits;            // n k records
    uint32_t* counts;      // n words or null
    uint32_t n, k;
    unsigned long long* stats;  // the counting instantiation's four words (include/hrt_testing.h); else unused
};

// ---- the host mirror ----
// True when the node bytes are a tree over (order, m): every child word reached from the root names a slot once or a leaf
// range inside n_order whose entries are below m.
inline bool host_tree_ok(const Tree& T, size_t slots, size_t n_order) {
    const auto leaf_ok = [&](uint32_t word) {
        const size_t first = (word >> 4) & 0x07FFFFFFu, cnt = word & 15u;
        if (first + cnt > n_order) return false;
        for (size_t s = 0; s < cnt; s++)
            if (T.order[first + s] >= T.m) return false;
        return true;
    };
    if ((T.root & LEAF_BIT) != 0u) return leaf_ok(T.root);
    if ((size_t)T.root >= slots) return false;
    std::vector<uint8_t> seen(slots, 0);
    std::vector<uint32_t> todo{T.root};
    seen[T.root] = 1;
    while (!todo.empty()) {
        const uint32_t node = todo.back();
        todo.pop_back();
        for (int s = 0; s < 2; s++) {
            const uint32_t w = T.hnodes[2 * (size_t)node + s].w;
            if ((w & LEAF_BIT) != 0u) {
                if (!leaf_ok(w)) return false;
            } else {
                if ((size_t)w >= slots || seen[w]) return false;
                seen[w] = 1;
                todo.push_back(w);
            }
        }
    }
    return true;
}

// n queries: the walk on T, or the flat definition for T.flat. hits: n k records; counts: n words or null (the walk then
// culls by the list, as the device does).
inline void host_multi(const Tree& T, const float* origins, const float* dirs, const float* tmax, const Hit* after, uint32_t n,
                       uint32_t k, Hit* hits, uint32_t* counts) {
    uint32_t stack[STACK];
    float lt[MAX_K];
    int32_t lj[MAX_K];
    for (uint32_t i = 0; i < n; i++) {
        const float* const o = origins + 3 * (size_t)i;
        const float* const d = dirs + 3 * (size_t)i;
        List L{lt, lj, 1u, k, 0u};
        uint32_t count = 0u;
        Tally tally{0u, 0u, 0u};
        const float tm = tmax ? tmax[i] : T_MISS;
        const bool cur = after != nullptr;
        const float at = cur ? after[i].t : 0.0f;
        const int32_t aj = cur ? after[i].prim : -1;
        if (counts) query<true, false>(T, o, d, tm, cur, at, aj, stack, 1u, L, count, tally);
        else query<false, false>(T, o, d, tm, cur, at, aj, stack, 1u, L, count, tally);
        for (uint32_t s = 0; s < k; s++) hits[(size_t)i * k + s] = make_record(T, o, d, L, s);
        if (counts) counts[i] = count;
    }
}

}  // namespace hrt_multihit
