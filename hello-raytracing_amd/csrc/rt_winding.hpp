// rt_winding.hpp — what the host (renderer.cpp: rt_host_tree_moments, rt_host_winding_numbers) and the device code
// (rt_winding.hip) of rt_winding_numbers share: the signed solid angle of a triangle as ONE inline function both compile,
// a written-out atan2, the moments of a subtree, the far-field rule, the walk, the flat definition and the launchers'
// arguments. Built with -ffp-contract=off like everything else, and no FMA is written here: every operation is rounded
// once, in the order written; IEEE division and square root (f32 and f64). No libm and no ocml call: host and device
// return the same bits (include/hrt.h rt_winding_numbers has the contract in words; DESIGN.md §7f the arguments).
//
//   w(p)       = (1 / 4 pi) sum_j Omega_j(p), the generalized winding number (Jacobson et al. 2013): 1 inside a closed
//                mesh wound outward, 0 outside, in between where the mesh is open. The sum S is kept in units of
//                Omega / 2 in one f64 per query, every term added in walk order; w = (float)(S / 2 pi).
//   triangle   half_angle(p, g): x0 = a - p, x1 = x0 + e1, x2 = x0 + e2 in f32; all nine components are multiplied by one
//                exact power of two taken from their largest magnitude, so that it lands in [1, 2) (the function is scale
//                invariant); l_k = |x_k|, num = x0 . (x1 x x2), den = l0 l1 l2 + (x0.x1) l2 + (x1.x2) l0 + (x2.x0) l1,
//                Omega / 2 = atan2(num, den) (Van Oosterom and Strackee 1983).
//                The scale comes from the triangle's own vectors, not from the query's D: the flat definition has to
//                answer without a tree, where there is no D, and a triangle that is tiny against D but close to the
//                point keeps its full weight this way.
//   no NaN     after the scaling every component is in (-4, 4) (the exponent is clamped to [1, 253], so the largest
//                finite f32 scales to just under 4): the dots are below 48, the lengths below 7, every product of den
//                below 343 and num below 3 * 4 * 32: no overflow, so num and den are finite and atan2_f32 of finite
//                arguments is in [-pi, pi]. Components that underflow give num = den = 0 and atan2(0, 0) = 0. A sum of
//                fewer than 2^32 such terms is finite in f64. A component that is not finite — a non-finite a, e1 or
//                e2, or a - p overflowing f32 — makes the triangle contribute exactly 0. A non-finite point never gets
//                here: its answer is the quiet NaN 0x7FC00000.
//   moments    per child of a node, from f64 sums over its triangles (tri_sums): An = e1 x e2, s = |An|,
//                g = 3 (a - rc) + e1 + e2; N = sum An, c = sum s g / (3 sum s), each rounded to f32 once; c is the box
//                centre and N = 0 when sum s is 0. A leaf child adds its order entries in order, a node child is
//                left + right. Should N or c not be finite in f32 the record holds c = NaN, N = 0, and the far-field
//                test below never takes that child whole.
//   far field  q = p - rc; for a child with moments (c, N) and decoded fp16 box [lo, hi]: d = c - q, L2 = |d|^2,
//                R2 = |max(c - lo, hi - c)|^2, all in f64 (the differences of f32 values are exact there). The child is
//                taken whole when L2 > beta^2 R2 — L > beta R without the roots; false for an infinite or NaN R2 and for
//                beta = +inf — and its term is N . d / (4 L2 sqrt(L2)) (Barill et al. 2018, first order).
//   walk       depth first, left child then right: a child is a dipole term if it is far, its triangles' terms if it is a
//                near leaf, and descended if it is a near node. When the left child is descended the node's index goes on
//                a stack of STACK words and its right child is judged when the index comes off again. A query that
//                would need one more word discards its sum and takes the flat definition (walk_sah's overflow rule,
//                for a sum).
//   flat       half_angle over all m triangles in index order, no dipoles: a tree without nodes (the root word is a
//                leaf), points outside D_MIN <= D <= D_MAX (D as rt_closest.hip has it), and the stack overflow.
//   atan2_f32  |error| <= ATAN2_ERR against the real function (tests/test_winding_abi.py sweeps it: twice the largest
//                error found, 2.73e-7); atan2(+-0, +-0) = 0; atan2(+-0, x < 0) = +-pi by the sign bit of the first argument.
#pragma once
#include <stdint.h>

#include "rt_lbvh.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HRT_WINDING_FN __host__ __device__ inline
#else
#define HRT_WINDING_FN inline
#endif

#include <vector>

namespace hrt_winding {

constexpr float D_MIN = 0x1p-40f, D_MAX = 0x1p60f;  // rt_closest.hpp's covered range
constexpr int STACK = 24;
constexpr uint32_t LEAF_BIT = hrt_lbvh::LEAF_BIT, NO_PARENT = hrt_lbvh::NO_PARENT;
constexpr float BETA_DEFAULT = 2.0f;
constexpr float ATAN2_ERR = 5.5e-7f;
constexpr double TWO_PI = 6.283185307179586;
constexpr uint32_t REC_FLOATS = 16;  // one node slot of the moments: per child c[3], N[3], 0, 0
constexpr uint32_t SUM_WORDS = 8;    // f64 per (node, side) in the climb's scratch: N[3], G[3], s, unused

using U4 = hrt_lbvh::U4;
using hrt_lbvh::f32_bits;
using hrt_lbvh::f32_finite;
using hrt_lbvh::f32_from_bits;
using hrt_lbvh::quiet_nan;
HRT_WINDING_FN float dot3(const float a[3], const float b[3]) {
    const float x = a[0] * b[0], y = a[1] * b[1], z = a[2] * b[2];
    return (x + y) + z;
}
HRT_WINDING_FN double half_to_f64(uint32_t b16) {
    const uint16_t b = (uint16_t)b16;
    _Float16 h;
    __builtin_memcpy(&h, &b, sizeof h);
    return (double)h;
}

// atan2(y, x) for arguments that are not NaN, in f32. t = min / max of the magnitudes in [0, 1] (inf / inf counts as 1);
// above tan(pi / 8) it is reduced to (t - 1) / (t + 1) with pi / 4 added; the odd polynomial is Cephes atanf's; then the
// octant, the half plane and the sign of y are put back. Never NaN.
HRT_WINDING_FN float atan2_f32(float y, float x) {
    const uint32_t yb = f32_bits(y), xb = f32_bits(x);
    const float ay = f32_from_bits(yb & 0x7FFFFFFFu), ax = f32_from_bits(xb & 0x7FFFFFFFu);
    const bool swap = ay > ax;
    const float mx = swap ? ay : ax, mn = swap ? ax : ay;
    if (!(mx > 0.0f)) return 0.0f;
    float t = mn / mx;
    if (!(t <= 1.0f)) t = 1.0f;
    float off = 0.0f;
    if (t > 0.41421357f) {
        const float tn = t - 1.0f, td = t + 1.0f;
        t = tn / td;
        off = 0.78539816f;
    }
    const float z = t * t;
    float s = 8.05374449538e-2f * z;
    s = s - 1.38776856032e-1f;
    s = s * z;
    s = s + 1.99777106478e-1f;
    s = s * z;
    s = s - 3.33329491539e-1f;
    s = s * z;
    s = s * t;
    s = s + t;
    float r = off + s;
    if (swap) r = 1.57079633f - r;
    if ((xb >> 31) != 0u) r = 3.14159265f - r;
    return (yb >> 31) != 0u ? -r : r;
}

// Omega / 2 of triangle g (a, e1, e2) seen from p.
HRT_WINDING_FN float half_angle(const float p[3], const float g[9]) {
    float x[9];
    uint32_t mb = 0u;
    for (int k = 0; k < 3; k++) {
        x[k] = g[k] - p[k];
        x[3 + k] = x[k] + g[3 + k];
        x[6 + k] = x[k] + g[6 + k];
    }
    for (int k = 0; k < 9; k++) {
        const uint32_t b = f32_bits(x[k]) & 0x7FFFFFFFu;
        mb = b > mb ? b : mb;
    }
    if (mb >= 0x7F800000u) return 0.0f;
    uint32_t e = mb >> 23;
    e = e < 1u ? 1u : (e > 253u ? 253u : e);
    const float sc = f32_from_bits((254u - e) << 23);  // 2^(127 - e)
    for (int k = 0; k < 9; k++) x[k] = x[k] * sc;
    const float *x0 = x, *x1 = x + 3, *x2 = x + 6;
    const float l0 = __builtin_sqrtf(dot3(x0, x0)), l1 = __builtin_sqrtf(dot3(x1, x1)), l2 = __builtin_sqrtf(dot3(x2, x2));
    float c[3];
    {
        const float a0 = x1[1] * x2[2], b0 = x1[2] * x2[1];
        const float a1 = x1[2] * x2[0], b1 = x1[0] * x2[2];
        const float a2 = x1[0] * x2[1], b2 = x1[1] * x2[0];
        c[0] = a0 - b0;
        c[1] = a1 - b1;
        c[2] = a2 - b2;
    }
    const float num = dot3(x0, c);
    const float d01 = dot3(x0, x1), d12 = dot3(x1, x2), d20 = dot3(x2, x0);
    const float t0 = (l0 * l1) * l2, t1 = d01 * l2, t2 = d12 * l0, t3 = d20 * l1;
    const float den = ((t0 + t1) + t2) + t3;
    return atan2_f32(num, den);
}

// ---- moments ----
struct Sums {
    double N[3], G[3], s;
};
HRT_WINDING_FN void sums_zero(Sums& a) {
    for (int k = 0; k < 3; k++) a.N[k] = a.G[k] = 0.0;
    a.s = 0.0;
}
HRT_WINDING_FN void sums_add(Sums& a, const Sums& b) {
    for (int k = 0; k < 3; k++) {
        a.N[k] = a.N[k] + b.N[k];
        a.G[k] = a.G[k] + b.G[k];
    }
    a.s = a.s + b.s;
}
// One triangle's share (nothing for a non-finite one). Products of two f32 values are exact in f64.
HRT_WINDING_FN void tri_sums_add(const float g[9], const float rc[3], Sums& a) {
    bool finite = true;
    for (int k = 0; k < 9; k++) finite = finite && f32_finite(g[k]);
    if (!finite) return;
    const double e1[3] = {(double)g[3], (double)g[4], (double)g[5]}, e2[3] = {(double)g[6], (double)g[7], (double)g[8]};
    double An[3];
    {
        const double a0 = e1[1] * e2[2], b0 = e1[2] * e2[1];
        const double a1 = e1[2] * e2[0], b1 = e1[0] * e2[2];
        const double a2 = e1[0] * e2[1], b2 = e1[1] * e2[0];
        An[0] = a0 - b0;
        An[1] = a1 - b1;
        An[2] = a2 - b2;
    }
    const double xx = An[0] * An[0], yy = An[1] * An[1], zz = An[2] * An[2];
    const double s = __builtin_sqrt((xx + yy) + zz);
    for (int k = 0; k < 3; k++) {
        const double rel = (double)g[k] - (double)rc[k];
        const double gk = ((3.0 * rel) + e1[k]) + e2[k];
        const double sg = s * gk;
        a.N[k] = a.N[k] + An[k];
        a.G[k] = a.G[k] + sg;
    }
    a.s = a.s + s;
}
// A leaf child: its order entries in order.
HRT_WINDING_FN void leaf_sums(uint32_t word, const uint32_t* order, const float* geo, const float rc[3], Sums& a) {
    sums_zero(a);
    const uint32_t first = (word >> 4) & 0x07FFFFFFu, cnt = word & 15u;
    for (uint32_t k = 0; k < cnt; k++) tri_sums_add(geo + 9 * (size_t)order[first + k], rc, a);
}
// The eight floats of one child: c[3], N[3], 0, 0. box: the child's U4 of the node.
HRT_WINDING_FN void child_record(const Sums& a, const U4& box, float rec[8]) {
    const uint32_t w[3] = {box.x, box.y, box.z};
    bool finite = true;
    for (int k = 0; k < 3; k++) {
        if (a.s > 0.0) {
            const double den = 3.0 * a.s;
            rec[k] = (float)(a.G[k] / den);
            rec[3 + k] = (float)a.N[k];
        } else {
            const double sum = half_to_f64(w[k] & 0xFFFFu) + half_to_f64(w[k] >> 16);
            rec[k] = (float)(0.5 * sum);
            rec[3 + k] = 0.0f;
        }
        finite = finite && f32_finite(rec[k]) && f32_finite(rec[3 + k]);
    }
    if (!finite)
        for (int k = 0; k < 3; k++) {
            rec[k] = quiet_nan();
            rec[3 + k] = 0.0f;
        }
    rec[6] = rec[7] = 0.0f;
}

// ---- the query ----
struct Tree {
    const U4* hnodes;       // two U4 per node slot (rt_lbvh.hpp pack_child)
    const float* moments;   // REC_FLOATS per node slot
    const uint32_t* order;  // the triangle index of every leaf position
    const float* geo;       // tri_geo: 9 m floats
    uint32_t m, root;       // triangles in geo; the root word
    float rc[3], rr_h;      // root centre; the radius bound of the fp16 boxes
};
struct Tally {
    uint32_t tri, dip, overflow, uncovered;
};

// The far-field rule for one child (box: its U4; rec: its eight floats). True: `term` is its dipole term.
HRT_WINDING_FN bool far_term(const U4& box, const float* rec, const float q[3], double beta2, double& term) {
    const uint32_t w[3] = {box.x, box.y, box.z};
    double dd[3], mm[3], nd[3];
    for (int k = 0; k < 3; k++) {
        const double c = (double)rec[k];
        const double d = c - (double)q[k];
        const double below = c - half_to_f64(w[k] & 0xFFFFu), above = half_to_f64(w[k] >> 16) - c;
        const double mk = below > above ? below : above;
        dd[k] = d * d;
        mm[k] = mk * mk;
        nd[k] = (double)rec[3 + k] * d;
    }
    const double L2 = (dd[0] + dd[1]) + dd[2], R2 = (mm[0] + mm[1]) + mm[2];
    if (!(L2 > beta2 * R2)) return false;
    const double n = (nd[0] + nd[1]) + nd[2];
    const double L3 = L2 * __builtin_sqrt(L2);
    term = n / (4.0 * L3);
    return true;
}

HRT_WINDING_FN double flat_sum(const Tree& T, const float p[3]) {
    double S = 0.0;
    for (uint32_t j = 0; j < T.m; j++) S = S + (double)half_angle(p, T.geo + 9 * (size_t)j);
    return S;
}

HRT_WINDING_FN float beta_of(float beta) { return beta == 0.0f ? BETA_DEFAULT : beta; }
// NaN, negative (-0 is 0) and (0, 1) are not a far-field factor.
HRT_WINDING_FN bool beta_ok(float beta) { return beta == 0.0f || beta >= 1.0f; }

// One query. stack: STACK words at `stride`. COUNT: tally the terms (the test-only instantiation).
template <bool COUNT>
HRT_WINDING_FN float query(const Tree& T, const float p[3], float beta, uint32_t* stack, uint32_t stride, Tally& t) {
    if (!(f32_finite(p[0]) && f32_finite(p[1]) && f32_finite(p[2]))) {
        t.uncovered = 1u;
        return quiet_nan();
    }
    bool flat = (T.root & LEAF_BIT) != 0u;
    double S = 0.0;
    if (!flat) {
        const float q[3] = {p[0] - T.rc[0], p[1] - T.rc[1], p[2] - T.rc[2]};
        const float D = __builtin_sqrtf(dot3(q, q)) * 1.001f + T.rr_h;
        if (D >= D_MIN && D <= D_MAX) {
            const double b = (double)beta_of(beta), beta2 = b * b;
            uint32_t node = T.root, side = 0u, sp = 0u;
            while (true) {  // child `side` of `node`
                const U4 box = T.hnodes[2 * (size_t)node + side];
                const float* const rec = T.moments + REC_FLOATS * (size_t)node + 8u * side;
                bool down = false;
                double term;
                if (far_term(box, rec, q, beta2, term)) {
                    S = S + term;
                    if (COUNT) t.dip += 1u;
                } else if ((box.w & LEAF_BIT) != 0u) {
                    const uint32_t first = (box.w >> 4) & 0x07FFFFFFu, cnt = box.w & 15u;
                    for (uint32_t k = 0; k < cnt; k++)
                        S = S + (double)half_angle(p, T.geo + 9 * (size_t)T.order[first + k]);
                    if (COUNT) t.tri += cnt;
                } else {
                    down = true;
                }
                if (down) {
                    if (side == 0u) {  // the right child waits
                        if (sp == (uint32_t)STACK) {
                            t.overflow = 1u;
                            flat = true;
                            break;
                        }
                        stack[sp * stride] = node;
                        sp++;
                    }
                    node = box.w;
                    side = 0u;
                } else if (side == 0u) {
                    side = 1u;
                } else {
                    if (sp == 0u) break;
                    sp--;
                    node = stack[sp * stride];
                    side = 1u;
                }
            }
        } else {
            t.uncovered = 1u;
            flat = true;
        }
    }
    if (flat) {
        S = flat_sum(T, p);
        if (COUNT) t.tri += T.m;
    }
    return (float)(S / TWO_PI);
}

// ---- the launchers' arguments (rt_winding.hip) ----
struct Launch {
    Tree tree;
    const float* points;  // 3 n floats
    float* out;           // n floats
    uint32_t n;
    float beta;
    unsigned long long* counts;  // the counting instantiation's five words (include/hrt_testing.h); else unused
};
struct MomentsLaunch {
    const U4* hnodes;
    const uint32_t* order;
    const float* geo;
    const uint32_t* parent;  // tb_parent: of node i at [i], node << 1 | side
    uint32_t slots;
    float rc[3];
    unsigned long long* sums;  // 2 slots SUM_WORDS f64 bit patterns
    uint32_t* arrivals;        // slots, zeroed per call
    float* moments;            // REC_FLOATS slots
};

// ---- the host mirrors ----
// The moments of every referenced node slot (the others stay 0), by the recursive definition without recursion. False
// when the bytes are not a tree over (order, geo): a child word past the slots or named twice, a leaf range past n_order,
// an order entry past m.
inline bool host_moments(const Tree& T, size_t slots, size_t n_order, float* out) {
    for (size_t i = 0; i < REC_FLOATS * slots; i++) out[i] = 0.0f;
    if ((T.root & LEAF_BIT) != 0u) return true;
    if ((size_t)T.root >= slots) return false;
    std::vector<Sums> total(slots);
    std::vector<uint8_t> state(slots, 0);
    std::vector<uint32_t> todo{T.root};
    state[T.root] = 1;
    const auto leaf_ok = [&](uint32_t word) {
        const size_t first = (word >> 4) & 0x07FFFFFFu, cnt = word & 15u;
        if (first + cnt > n_order) return false;
        for (size_t k = 0; k < cnt; k++)
            if (T.order[first + k] >= T.m) return false;
        return true;
    };
    while (!todo.empty()) {
        const uint32_t node = todo.back();
        const U4 box[2] = {T.hnodes[2 * (size_t)node], T.hnodes[2 * (size_t)node + 1]};
        if (state[node] == 1) {
            state[node] = 2;
            for (int s = 0; s < 2; s++) {
                const uint32_t w = box[s].w;
                if ((w & LEAF_BIT) != 0u) {
                    if (!leaf_ok(w)) return false;
                } else {
                    if ((size_t)w >= slots || state[w] != 0) return false;
                    state[w] = 1;
                    todo.push_back(w);
                }
            }
            continue;
        }
        todo.pop_back();
        Sums side[2];
        for (int s = 0; s < 2; s++) {
            if ((box[s].w & LEAF_BIT) != 0u) leaf_sums(box[s].w, T.order, T.geo, T.rc, side[s]);
            else side[s] = total[box[s].w];
            child_record(side[s], box[s], out + REC_FLOATS * (size_t)node + 8 * s);
        }
        total[node] = side[0];
        sums_add(total[node], side[1]);
    }
    return true;
}

// n queries on the tree (T.moments set), or the flat definition for a T whose root word is a leaf.
inline void host_winding(const Tree& T, const float* points, uint32_t n, float beta, float* out) {
    uint32_t stack[STACK];
    for (uint32_t i = 0; i < n; i++) {
        Tally t{0u, 0u, 0u, 0u};
        out[i] = query<false>(T, points + 3 * (size_t)i, beta, stack, 1u, t);
    }
}

}  // namespace hrt_winding
