// rt_lbvh.hpp — what the host (renderer.cpp, rt_host_lbvh_build) and the device code (rt_lbvh.hip) of
// rt_set_triangles_device share: every arithmetic rule of the LBVH builder as ONE inline function both compile, the
// builder itself on the host (host_build, the mirror the tests compare the device tree with, bit for bit), and the
// launcher's arguments. Built with -ffp-contract=off like everything else, and no FMA is written here.
//
// The rules (include/hrt.h rt_set_triangles_device has them in words). They make the tree a pure function
// of the triangle array: nothing depends on which lane, wave or workgroup gets somewhere first.
//   prep      e1 = b - a, e2 = c - a in f32 (the TriDev / tri_geo record of rt_set_bvh). The box is over a, a + e1, a + e2
//             summed in f64 (exact), with -0 turned into +0; the centroid is (v0 + v1 + v2) / 3.0 in f64. A triangle with
//             a non-finite a, e1 or e2 is left out of the tree (key 0xFFFFFFFF).
//   root box  the union of the finite triangles' f64 boxes: min and max of f64 values without -0 or NaN are exact and
//             do not depend on the order (the device takes them with integer atomics on ordered bit patterns: f64_key).
//   keys      30-bit Morton code, 10 bits per axis, of the cell (c - lo) / (hi - lo) * 1024.0 in f64; an axis without
//             extent is cell 0; NaN and everything <= 0 give 0, everything >= 1024 gives 1023 (morton_key).
//   sort      stable by key (hrt_launch_regroup, mode 2): equal keys keep triangle order.
//   topology  Karras' construction over the m' finite triangles' sorted keys: delta(i, j) is the length of the common
//             prefix of the keys, and 32 + clz(i ^ j) for equal keys (topology). Node 0 is the root. A child whose range
//             holds <= LEAF_MAX positions is a leaf word LEAF_BIT | first << 4 | count; the internal slots below it stay
//             unreferenced and zero. m' = 0: root word LEAF_BIT; m' <= LEAF_MAX: one leaf word, no nodes.
//   fit       the f64 box of a node is the union of its children's; a referenced node's two child boxes are packed as
//             the host's SAH tree packs them (pack_child: down / up to f32 with the extra ulp, relative to the f32 root
//             centre with one more ulp outward, fp16 outward).
//   refit     (rt_refit_triangles_device, rt_host_lbvh_refit) prep and fit over another array of the same triangles, on
//             the topology as it stands: the same set of finite triangles is asked for, nothing else.
//   cost      (rt_get_tri_tree_cost, rt_host_lbvh_cost) cost_node: integers from the packed boxes alone.
//   ploc      (builder RT_TREE_PLOC: rt_set_triangles_device_with, rt_host_lbvh_build_with; kernels in rt_ploc.hip) a second
//             topology over the same sorted order: locally-ordered clustering (Meister and Bittner 2018), stated at "the
//             PLOC topology" below as a pure function. It writes what Karras' construction writes (order, parent links,
//             child words, node 0 the root), so the fit, the refit, the cost and the walk are the ones above.
#pragma once
#include <stdint.h>

#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HRT_LBVH_FN __host__ __device__ inline
#else
#define HRT_LBVH_FN inline
#endif

namespace hrt_lbvh {

constexpr uint32_t LEAF_BIT = 0x80000000u;   // (BVH_LEAF_BIT of rt_device.hpp / host/sphere_bvh.hpp)
#ifndef HRT_LBVH_LEAF_MAX
#define HRT_LBVH_LEAF_MAX 4  // (a build with 1 is scripts/bench_lbvh.py's comparison, never the product)
#endif
constexpr uint32_t LEAF_MAX = HRT_LBVH_LEAF_MAX;
constexpr uint32_t KEY_NONFINITE = 0xFFFFFFFFu;
constexpr uint32_t NO_PARENT = 0xFFFFFFFFu;
static_assert(LEAF_MAX >= 1 && LEAF_MAX <= 15, "a leaf word holds its count in 4 bits");

struct U4 {
    uint32_t x, y, z, w;
};

// ---- bit patterns ----
HRT_LBVH_FN uint32_t f32_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
HRT_LBVH_FN float f32_from_bits(uint32_t u) {
    float x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}
HRT_LBVH_FN uint64_t f64_bits(double x) {
    uint64_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}
HRT_LBVH_FN double f64_from_bits(uint64_t u) {
    double x;
    __builtin_memcpy(&x, &u, sizeof x);
    return x;
}
HRT_LBVH_FN bool f32_finite(float x) { return (f32_bits(x) & 0x7F800000u) != 0x7F800000u; }
HRT_LBVH_FN float quiet_nan() { return f32_from_bits(0x7FC00000u); }

// An unsigned key with the order of the f64 values (no NaN): a < b exactly when f64_key(a) < f64_key(b).
HRT_LBVH_FN uint64_t f64_key(double x) {
    const uint64_t u = f64_bits(x);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
HRT_LBVH_FN double f64_from_key(uint64_t k) { return f64_from_bits((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k); }

HRT_LBVH_FN double dmin(double a, double b) { return b < a ? b : a; }
HRT_LBVH_FN double dmax(double a, double b) { return b > a ? b : a; }

// The next f32 towards +inf (up) or -inf: std::nextafter(f, +-INFINITY) for every f but NaN.
HRT_LBVH_FN float f32_step(float f, bool up) {
    const uint32_t b = f32_bits(f);
    if ((b & 0x7FFFFFFFu) == 0u) return f32_from_bits(up ? 0x00000001u : 0x80000001u);  // +-0 -> smallest subnormal
    const bool neg = (b >> 31) != 0u;
    if ((b & 0x7FFFFFFFu) == 0x7F800000u && up != neg) return f;  // the infinity on that side stays
    return f32_from_bits(up != neg ? b + 1u : b - 1u);
}

// f32 bounds that contain the f64 value, with one extra ulp outward (host/tri_bvh.cpp's down / up).
HRT_LBVH_FN float f32_outward(double v, bool up) {
    float f = (float)v;
    if (up ? (double)f < v : (double)f > v) f = f32_step(f, up);
    return f32_step(f, up);
}

// A half that bounds the f32 value on the given side (renderer.cpp's packers use these too).
HRT_LBVH_FN uint16_t f16_bits(_Float16 h) {
    uint16_t u;
    __builtin_memcpy(&u, &h, sizeof u);
    return u;
}
HRT_LBVH_FN _Float16 f16_from_bits(uint16_t b) {
    _Float16 h;
    __builtin_memcpy(&h, &b, sizeof h);
    return h;
}
HRT_LBVH_FN _Float16 f16_step(_Float16 h, bool up) {
    uint16_t b = f16_bits(h);
    if ((b & 0x7FFFu) == 0u) return f16_from_bits(up ? 0x0001u : 0x8001u);  // +-0 -> smallest subnormal
    const bool neg = (b & 0x8000u) != 0u;
    b = (uint16_t)((up != neg) ? b + 1u : b - 1u);
    return f16_from_bits(b);
}
HRT_LBVH_FN uint32_t f16_dir(float x, bool up) {
    _Float16 h = (_Float16)x;
    if (up ? (float)h < x : (float)h > x) h = f16_step(h, up);
    return f16_bits(h);
}

// One bound of a packed box: the f32 bound `v` relative to the f32 centre coordinate, one ulp outward, as a half
// outward (renderer.cpp pack_bvh_hnodes).
HRT_LBVH_FN uint32_t rel_f16(float v, float center, bool up) {
    const float f = f32_step((float)((double)v - (double)center), up);
    return f16_dir(f, up);
}

// One child of a node as the walk reads it: per axis [min | max << 16] halves, then the child word.
HRT_LBVH_FN U4 pack_child(const double lo[3], const double hi[3], const float rc[3], uint32_t word) {
    uint32_t a[3];
    for (int k = 0; k < 3; k++)
        a[k] = rel_f16(f32_outward(lo[k], false), rc[k], false) | rel_f16(f32_outward(hi[k], true), rc[k], true) << 16;
    return U4{a[0], a[1], a[2], word};
}

// The f32 centre of the root box (host/tri_bvh.cpp build_tri_bvh).
HRT_LBVH_FN float root_center(double lo, double hi) { return (float)(0.5 * (lo + hi)); }

// ---- prep ----
// aee: a, e1, e2 (9 floats). False for a triangle that stays out of the tree; else its f64 box and centroid.
HRT_LBVH_FN bool tri_bounds(const float aee[9], double lo[3], double hi[3], double cen[3]) {
    bool finite = true;
    for (int k = 0; k < 9; k++) finite = finite && f32_finite(aee[k]);
    if (!finite) return false;
    for (int k = 0; k < 3; k++) {
        const double v0 = (double)aee[k] + 0.0;  // (-0 -> +0)
        const double v1 = (double)aee[k] + (double)aee[3 + k] + 0.0;  // exact in f64
        const double v2 = (double)aee[k] + (double)aee[6 + k] + 0.0;
        lo[k] = dmin(dmin(v0, v1), v2);
        hi[k] = dmax(dmax(v0, v1), v2);
        cen[k] = (v0 + v1 + v2) / 3.0;
    }
    return true;
}

// ---- keys ----
HRT_LBVH_FN uint32_t cell_axis(double c, double lo, double hi) {
    const double ext = hi - lo;
    if (!(ext > 0.0)) return 0u;
    const double f = (c - lo) / ext * 1024.0;
    if (!(f > 0.0)) return 0u;
    if (f >= 1024.0) return 1023u;
    return (uint32_t)f;
}
// Bit i of q (10 bits) to bit 3 i.
HRT_LBVH_FN uint32_t spread3(uint32_t q) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < 10u; i++) r |= ((q >> i) & 1u) << (3u * i);
    return r;
}
HRT_LBVH_FN uint32_t morton_key(const double cen[3], const double rlo[3], const double rhi[3]) {
    return spread3(cell_axis(cen[0], rlo[0], rhi[0])) | spread3(cell_axis(cen[1], rlo[1], rhi[1])) << 1 |
           spread3(cell_axis(cen[2], rlo[2], rhi[2])) << 2;
}

// ---- topology ----
HRT_LBVH_FN int clz32(uint32_t x) { return x ? __builtin_clz(x) : 32; }
// Common-prefix length of sorted positions i and j; -1 outside [0, m).
HRT_LBVH_FN int delta(const uint32_t* keys, int m, int i, int j) {
    if (j < 0 || j >= m) return -1;
    const uint32_t a = keys[i], b = keys[j];
    if (a != b) return clz32(a ^ b);
    return 32 + clz32((uint32_t)i ^ (uint32_t)j);
}
// Internal node i (0 <= i < m - 1, m >= 2) of Karras' tree: its range [first, last] of sorted positions and the
// split: the left child covers [first, split], the right one [split + 1, last].
HRT_LBVH_FN void topology(const uint32_t* keys, int m, int i, int& first, int& last, int& split) {
    const int d = delta(keys, m, i, i + 1) > delta(keys, m, i, i - 1) ? 1 : -1;
    const int dmin_ = delta(keys, m, i, i - d);
    int lmax = 2;
    while (delta(keys, m, i, i + lmax * d) > dmin_) lmax *= 2;
    int l = 0;
    for (int t = lmax / 2; t >= 1; t /= 2)
        if (delta(keys, m, i, i + (l + t) * d) > dmin_) l += t;
    const int j = i + l * d;
    const int dnode = delta(keys, m, i, j);
    int s = 0, t = l;
    do {
        t = (t + 1) >> 1;
        if (delta(keys, m, i, i + (s + t) * d) > dnode) s += t;
    } while (t > 1);
    split = i + s * d + (d < 0 ? -1 : 0);
    first = d > 0 ? i : j;
    last = d > 0 ? j : i;
}
// The child word of a child covering [first, last]: `node` is the internal node it would be.
HRT_LBVH_FN uint32_t child_word(int first, int last, int node) {
    const uint32_t count = (uint32_t)(last - first + 1);
    return count <= LEAF_MAX ? (LEAF_BIT | (uint32_t)first << 4 | count) : (uint32_t)node;
}
// The root word for m finite triangles.
HRT_LBVH_FN uint32_t root_word(uint32_t m) { return m <= LEAF_MAX ? (LEAF_BIT | m) : 0u; }
// Internal nodes the hnode array holds (referenced or not) for m finite triangles.
HRT_LBVH_FN uint32_t node_slots(uint32_t m) { return m <= LEAF_MAX ? 0u : m - 1u; }

// ---- tree cost (rt_get_tri_tree_cost, rt_host_lbvh_cost) ----
// A pure function of a tree's bytes, in integers: per child of a referenced node the half-area of its decoded fp16 box over
// the half-area R of the root node's two children's union, as a 16.16 fixed-point number. Any tree of the node format.
// One extent of a packed box: hi - lo of the two halves (exact in f64); nothing for an empty or NaN extent, and the
// largest extent two finite halves have for anything beyond it (inf halves).
HRT_LBVH_FN double cost_extent(uint32_t word) {
    const double lo = (double)f16_from_bits((uint16_t)(word & 0xFFFFu)), hi = (double)f16_from_bits((uint16_t)(word >> 16));
    const double e = hi - lo;
    if (!(e > 0.0)) return 0.0;
    return e > 131008.0 ? 131008.0 : e;
}
HRT_LBVH_FN double cost_half_area(double ex, double ey, double ez) {
    const double xy = ex * ey, yz = ey * ez, zx = ez * ex;  // (each rounded: no FMA)
    const double s = xy + yz;
    return s + zx;
}
HRT_LBVH_FN double cost_child_area(const U4& c) { return cost_half_area(cost_extent(c.x), cost_extent(c.y), cost_extent(c.z)); }
// R: the same expression over the union of the root node's two child boxes.
HRT_LBVH_FN double cost_root_area(const U4& l, const U4& r) {
    const uint32_t a[3] = {l.x, l.y, l.z}, b[3] = {r.x, r.y, r.z};
    double e[3];
    for (int k = 0; k < 3; k++) {
        const double lo = dmin((double)f16_from_bits((uint16_t)(a[k] & 0xFFFFu)), (double)f16_from_bits((uint16_t)(b[k] & 0xFFFFu)));
        const double hi = dmax((double)f16_from_bits((uint16_t)(a[k] >> 16)), (double)f16_from_bits((uint16_t)(b[k] >> 16)));
        const double d = hi - lo;
        e[k] = !(d > 0.0) ? 0.0 : d > 131008.0 ? 131008.0 : d;
    }
    return cost_half_area(e[0], e[1], e[2]);
}
HRT_LBVH_FN uint64_t cost_q(double A, double R) {
    if (!(R > 0.0)) return 0u;
    const double v = A / R * 65536.0;  // (A, R finite and >= 0: never NaN)
    return v >= 4294967296.0 ? 4294967296ull : (uint64_t)v;
}
// One node slot's share: cost[0] q of node children, [1] q x count of leaf children, [2] referenced nodes, [3] leaf entries.
HRT_LBVH_FN void cost_node(const U4& l, const U4& r, double R, uint64_t cost[4]) {
    if (l.w == 0u) return;  // a slot no child word names
    cost[2] += 1u;
    const U4* const c[2] = {&l, &r};
    for (int s = 0; s < 2; s++) {
        const uint64_t q = cost_q(cost_child_area(*c[s]), R);
        if ((c[s]->w & LEAF_BIT) != 0u) {
            const uint64_t count = c[s]->w & 15u;
            cost[1] += q * count;
            cost[3] += count;
        } else {
            cost[0] += q;
        }
    }
}

// ---- the PLOC topology (builder 1) ----
// Clusters: an f64 box and a child word each, at first one per sorted position p (tri_bounds of triangle order[p],
// LEAF_BIT | p << 4 | 1: every leaf holds one triangle). Iteration t = 0, 1, ... over the list of c >= 2 clusters:
//   distance   d(i, j) = cost_half_area of the union box's extents (each operation rounded in f64; bitwise symmetric: the
//              boxes hold no NaN and no -0). Flat mode: when t + clog2(c) >= PLOC_LEVELS, d = 0 for every pair.
//   neighbour  nn(i) = the j in [i - PLOC_RADIUS, i + PLOC_RADIUS] inside the list, j != i, with the smallest
//              (d(i, j), i ^ j): a symmetric key, strict among the pairs that share an endpoint, so a mutual pair exists.
//   merge      i < j merge when nn(i) = j and nn(j) = i. With k such pairs and `next` node ids not given out yet (m' - 1
//              at first), the s-th pair in order of i becomes node next - k + s, then next -= k: the last merge is node 0
//              and a child's id is above its parent's. Left word = cluster i's, right word = cluster j's; the merged
//              cluster (union box, word = id) takes i's place, j is dropped, the others keep their order.
// A flat iteration leaves ceil(c / 2) clusters, so there are at most PLOC_LEVELS iterations, and a node made in iteration t
// has height <= t + 1: no leaf has more than 64 nodes above it, the level cap of the fit kernels.
constexpr int PLOC_RADIUS = 8;
constexpr uint32_t PLOC_LEVELS = 64;
constexpr uint32_t PLOC_TAIL = 1024;  // (device) a list this short is finished by one workgroup in one launch
struct Cluster {                      // 56 B: two lists of n fit in the fit's box slots (BOX_WORDS u64 per side)
    double lo[3], hi[3];
    uint32_t word, unused;
};
HRT_LBVH_FN uint32_t ploc_clog2(uint32_t c) { return c <= 1u ? 0u : 32u - (uint32_t)clz32(c - 1u); }
HRT_LBVH_FN bool ploc_flat(uint32_t t, uint32_t c) { return t + ploc_clog2(c) >= PLOC_LEVELS; }
HRT_LBVH_FN double ploc_distance(const double alo[3], const double ahi[3], const double blo[3], const double bhi[3]) {
    double e[3];
    for (int k = 0; k < 3; k++) e[k] = dmax(ahi[k], bhi[k]) - dmin(alo[k], blo[k]);
    return cost_half_area(e[0], e[1], e[2]);
}
// nn(i) in a list of c >= 2 clusters; box(j, lo, hi) gives cluster j's box.
template <class BoxOf>
HRT_LBVH_FN int ploc_nearest(const BoxOf& box, int i, int c, bool flat) {
    double lo[3], hi[3];
    box(i, lo, hi);
    const int j0 = i - PLOC_RADIUS < 0 ? 0 : i - PLOC_RADIUS, j1 = i + PLOC_RADIUS > c - 1 ? c - 1 : i + PLOC_RADIUS;
    int best = -1;
    double bd = 0.0;
    for (int j = j0; j <= j1; j++) {
        if (j == i) continue;
        double d = 0.0;
        if (!flat) {
            double olo[3], ohi[3];
            box(j, olo, ohi);
            d = ploc_distance(lo, hi, olo, ohi);
        }
        if (best < 0 || d < bd || (d == bd && (i ^ j) < (i ^ best))) {
            best = j;
            bd = d;
        }
    }
    return best;
}
// The link slot of the cluster with child word `word`: a node's own index, a leaf's position after `leaf_base` (m' on the
// host, n on the device: HostTopology::parent, Launch::parent).
HRT_LBVH_FN uint32_t ploc_link_slot(uint32_t word, uint32_t leaf_base) {
    return (word & LEAF_BIT) != 0u ? leaf_base + ((word & ~LEAF_BIT) >> 4) : word;
}

// ---- the device build's memory (rt_lbvh.hip; renderer.cpp allocates) ----
constexpr uint32_t STAT_WORDS = 16;  // u64 each: [0..2] ~f64_key of the root minima, [3..5] f64_key of the root maxima,
                                     // [6] finite triangles, [7] triangles with a bad material index, [8] depth,
                                     // [9] (refit) triangles whose finiteness is not the live tree's,
                                     // [10] (PLOC) clusters left after an iteration; iterations run, once the tail is done,
                                     // [11] (PLOC) pairs merged by an iteration; flat iterations, once the tail is done,
                                     // [12..15] (rt_get_tri_tree_cost) the four cost words
constexpr uint32_t BOX_WORDS = 8;    // u64 per (node, side): lo xyz, hi xyz as f64 bits, the subtree's height, unused
struct Launch {
    const void* tris64;       // the caller's n Triangle records (device)
    uint32_t n, n_mats;
    void* tris_out;           // n TriDev
    float* geo_out;           // 9 n floats
    U4* hnodes;               // 2 max(n - 1, 1) entries
    uint32_t* order;          // n: the sorted triangle indices
    uint32_t* keys;           // n
    uint32_t* keys_sorted;    // n
    uint32_t* parent;         // 2 n: of internal node i at [i], of sorted position p at [n + p]: node << 1 | side
    uint32_t* arrivals;       // n, zeroed per call
    uint64_t* boxes;          // 2 n BOX_WORDS
    uint64_t* stat;           // STAT_WORDS
    uint32_t* sort_entries;   // the renderer's regroup scratch (rt_regroup.hpp Launch)
    uint32_t* sort_counts;
};
// rt_refit_triangles_device: the live tree's topology is read, the staging set is written (k_lbvh_refit_prep, _fit).
struct Refit {
    const void* tris64;          // the caller's n Triangle records (device)
    uint32_t n, n_mats, m;       // m: the live tree's finite triangles (leaf positions)
    const float* geo_live;       // 9 n floats: the live tri_geo, for the finiteness comparison
    const U4* hnodes_live;       // the live node array: the child words
    const uint32_t* order;       // m: the live sorted triangle indices
    const uint32_t* parent;      // 2 n: the live parent links, laid out as Launch::parent
    void* tris_out;              // staging: n TriDev
    float* geo_out;              // staging: 9 n floats
    U4* hnodes;                  // staging: 2 (m - 1) entries, zeroed per call (by the prep)
    uint32_t* arrivals;          // n, the first m - 1 zeroed per call (by the prep)
    uint64_t* boxes;             // 2 n BOX_WORDS
    uint64_t* stat;              // STAT_WORDS, zeroed per call
};

// ---- the builder on the host ----
struct HostTree {
    std::vector<U4> hnodes;       // 2 per node slot
    std::vector<uint32_t> order;  // the finite triangles' indices in key order
    uint32_t root = LEAF_BIT, depth = 0, finite = 0;
    uint32_t iterations = 0, flat = 0;  // (PLOC) of the topology
    float rc[3] = {0, 0, 0};
    float radius = 0;
};

// Root centre and radius from the f64 root box (host/tri_bvh.cpp build_tri_bvh's formulas).
inline void root_sphere(const double lo[3], const double hi[3], float rc[3], float* radius) {
    double diag2 = 0.0;
    for (int k = 0; k < 3; k++) {
        rc[k] = root_center(lo[k], hi[k]);
        const double h = dmax(hi[k] - (double)rc[k], (double)rc[k] - lo[k]);
        diag2 += h * h;
    }
    *radius = f32_outward(std::sqrt(diag2) * (1.0 + 1e-6), true);
}

// The build in two halves, so that the refit (rt_host_lbvh_refit) shares them: host_topology (builder 0) or
// host_topology_ploc (builder 1) is everything that depends on the keys (which triangles are in the tree, their order, the
// parent links, the child words), host_fit everything that depends on positions alone (the root sphere, the packed boxes,
// the depth) and nothing on how the topology was made.
struct HostTopology {
    std::vector<uint8_t> fin;     // per triangle: in the tree
    std::vector<uint32_t> order;  // the finite triangles' indices in key order
    std::vector<uint32_t> parent; // 2 m: of internal node i at [i], of sorted position p at [m + p]: node << 1 | side
    std::vector<U4> words;        // 2 per node slot: only the child words (w) of the referenced nodes are set
    uint32_t finite = 0;
    uint32_t iterations = 0, flat = 0;  // (PLOC) iterations run, and how many of them in flat mode
};

// Everything up to the sort, which the builders share: the finite set, the keys in the root box, the stable order.
// aee: 9 floats per triangle (a, e1, e2), as rt_set_bvh and the prep kernel make them. keys: per triangle.
inline HostTopology host_sorted(const float* aee, uint32_t n, std::vector<uint32_t>& keys) {
    HostTopology P;
    keys.assign(n, KEY_NONFINITE);
    P.fin.assign(n, 0);
    double rlo[3] = {INFINITY, INFINITY, INFINITY}, rhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    std::vector<double> cen(3 * (size_t)n);
    for (uint32_t j = 0; j < n; j++) {
        double lo[3], hi[3];
        if (!tri_bounds(aee + 9 * (size_t)j, lo, hi, &cen[3 * (size_t)j])) continue;
        P.fin[j] = 1;
        P.finite++;
        for (int k = 0; k < 3; k++) {
            rlo[k] = dmin(rlo[k], lo[k]);
            rhi[k] = dmax(rhi[k], hi[k]);
        }
    }
    const uint32_t m = P.finite;
    if (m == 0) return P;
    for (uint32_t j = 0; j < n; j++)
        if (P.fin[j]) keys[j] = morton_key(&cen[3 * (size_t)j], rlo, rhi);
    // stable counting sort by key, 4 passes of 8 bits (any stable sort gives this order)
    std::vector<uint32_t> idx(n), tmp(n);
    for (uint32_t j = 0; j < n; j++) idx[j] = j;
    for (uint32_t shift = 0; shift < 32u; shift += 8u) {
        size_t count[257] = {0};
        for (uint32_t i = 0; i < n; i++) count[((keys[idx[i]] >> shift) & 255u) + 1u]++;
        for (int d = 0; d < 256; d++) count[d + 1] += count[d];
        for (uint32_t i = 0; i < n; i++) tmp[count[(keys[idx[i]] >> shift) & 255u]++] = idx[i];
        idx.swap(tmp);
    }
    P.order.assign(idx.begin(), idx.begin() + m);
    return P;
}

// Builder 0: Karras' topology.
inline HostTopology host_topology(const float* aee, uint32_t n) {
    std::vector<uint32_t> keys;
    HostTopology P = host_sorted(aee, n, keys);
    const uint32_t m = P.finite;
    if (m <= LEAF_MAX) return P;
    std::vector<uint32_t> ks(m);
    for (uint32_t p = 0; p < m; p++) ks[p] = keys[P.order[p]];
    const uint32_t nodes = m - 1u;
    P.words.assign(2 * (size_t)nodes, U4{0u, 0u, 0u, 0u});
    P.parent.assign(2 * (size_t)m, NO_PARENT);
    for (uint32_t i = 0; i < nodes; i++) {
        int first, last, split;
        topology(ks.data(), (int)m, (int)i, first, last, split);
        if (split == first) P.parent[m + (uint32_t)split] = i << 1;
        else P.parent[(uint32_t)split] = i << 1;
        if (split + 1 == last) P.parent[m + (uint32_t)split + 1u] = i << 1 | 1u;
        else P.parent[(uint32_t)split + 1u] = i << 1 | 1u;
        if ((uint32_t)(last - first + 1) > LEAF_MAX) {
            P.words[2 * (size_t)i].w = child_word(first, split, split);
            P.words[2 * (size_t)i + 1].w = child_word(split + 1, last, split + 1);
        }
    }
    return P;
}

// Builder 1: the PLOC topology (the rules above), one iteration after the other. All m' - 1 slots end up referenced.
inline HostTopology host_topology_ploc(const float* aee, uint32_t n) {
    std::vector<uint32_t> keys;
    HostTopology P = host_sorted(aee, n, keys);
    const uint32_t m = P.finite;
    if (m <= LEAF_MAX) return P;
    P.words.assign(2 * (size_t)(m - 1u), U4{0u, 0u, 0u, 0u});
    P.parent.assign(2 * (size_t)m, NO_PARENT);
    std::vector<Cluster> cur(m), nxt;
    for (uint32_t p = 0; p < m; p++) {
        double cen[3];
        tri_bounds(aee + 9 * (size_t)P.order[p], cur[p].lo, cur[p].hi, cen);  // (true: a finite one)
        cur[p].word = LEAF_BIT | p << 4 | 1u;
        cur[p].unused = 0u;
    }
    std::vector<int> nn;
    uint32_t next = m - 1u;
    while (cur.size() >= 2) {
        const int c = (int)cur.size();
        const bool flat = ploc_flat(P.iterations, (uint32_t)c);
        const auto box = [&](int j, double lo[3], double hi[3]) {
            for (int k = 0; k < 3; k++) {
                lo[k] = cur[(size_t)j].lo[k];
                hi[k] = cur[(size_t)j].hi[k];
            }
        };
        nn.resize((size_t)c);
        uint32_t pairs = 0;
        for (int i = 0; i < c; i++) nn[(size_t)i] = ploc_nearest(box, i, c, flat);
        for (int i = 0; i < c; i++) pairs += nn[(size_t)i] > i && nn[(size_t)nn[(size_t)i]] == i;
        uint32_t id = next - pairs;
        next -= pairs;
        nxt.clear();
        for (int i = 0; i < c; i++) {
            const int j = nn[(size_t)i];
            const bool mutual = nn[(size_t)j] == i;
            if (mutual && j < i) continue;  // the higher partner: dropped
            Cluster a = cur[(size_t)i];
            if (mutual) {
                const Cluster& b = cur[(size_t)j];
                P.words[2 * (size_t)id].w = a.word;
                P.words[2 * (size_t)id + 1].w = b.word;
                P.parent[ploc_link_slot(a.word, m)] = id << 1;
                P.parent[ploc_link_slot(b.word, m)] = id << 1 | 1u;
                for (int k = 0; k < 3; k++) {
                    a.lo[k] = dmin(a.lo[k], b.lo[k]);
                    a.hi[k] = dmax(a.hi[k], b.hi[k]);
                }
                a.word = id++;
            }
            nxt.push_back(a);
        }
        cur.swap(nxt);
        P.iterations++;
        P.flat += flat ? 1u : 0u;
    }
    return P;
}

inline HostTopology host_topology_of(const float* aee, uint32_t n, uint32_t builder) {
    return builder == 1u ? host_topology_ploc(aee, n) : host_topology(aee, n);
}

// The boxes of `aee` on the topology P (of the same n triangles). False, with T untouched past its defaults, when a
// triangle of aee is finite where P's was not or the other way round.
inline bool host_fit(const HostTopology& P, const float* aee, uint32_t n, HostTree& T) {
    struct Box {
        double lo[3], hi[3];
    };
    std::vector<Box> tb(n);
    double rlo[3] = {INFINITY, INFINITY, INFINITY}, rhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t j = 0; j < n; j++) {
        double cen[3];
        const bool fin = tri_bounds(aee + 9 * (size_t)j, tb[j].lo, tb[j].hi, cen);
        if (fin != (P.fin[j] != 0)) return false;
        if (!fin) continue;
        for (int k = 0; k < 3; k++) {
            rlo[k] = dmin(rlo[k], tb[j].lo[k]);
            rhi[k] = dmax(rhi[k], tb[j].hi[k]);
        }
    }
    const uint32_t m = P.finite;
    T.finite = m;
    T.root = root_word(m);
    T.iterations = P.iterations;
    T.flat = P.flat;
    if (m == 0) return true;
    root_sphere(rlo, rhi, T.rc, &T.radius);
    T.order = P.order;
    if (m <= LEAF_MAX) return true;
    const uint32_t nodes = m - 1u;
    T.hnodes = P.words;
    const std::vector<uint32_t>& parent = P.parent;
    // the fit, as the device does it: every position climbs; at a parent the first arriver leaves its box and stops
    struct Side {
        Box b;
        uint32_t height;
    };
    std::vector<Side> sides(2 * (size_t)nodes);
    std::vector<uint8_t> arrived(nodes, 0);
    for (uint32_t p = 0; p < m; p++) {
        Box b = tb[T.order[p]];
        uint32_t h = 0, link = parent[m + p];
        while (link != NO_PARENT) {
            const uint32_t node = link >> 1, side = link & 1u;
            sides[2 * (size_t)node + side] = Side{b, h};
            if (!arrived[node]++) break;
            const Side& o = sides[2 * (size_t)node + (side ^ 1u)];
            U4& left = T.hnodes[2 * (size_t)node];
            if (left.w != 0u) {
                const Side& L = sides[2 * (size_t)node], &R = sides[2 * (size_t)node + 1];
                left = pack_child(L.b.lo, L.b.hi, T.rc, left.w);
                T.hnodes[2 * (size_t)node + 1] = pack_child(R.b.lo, R.b.hi, T.rc, T.hnodes[2 * (size_t)node + 1].w);
                h = 1u + (h > o.height ? h : o.height);
            }
            for (int k = 0; k < 3; k++) {
                b.lo[k] = dmin(b.lo[k], o.b.lo[k]);
                b.hi[k] = dmax(b.hi[k], o.b.hi[k]);
            }
            if (node == 0u) T.depth = h;
            link = parent[node];
        }
    }
    return true;
}

// builder: RT_TREE_LBVH (0) or RT_TREE_PLOC (1) of include/hrt.h.
inline HostTree host_build(const float* aee, uint32_t n, uint32_t builder = 0u) {
    HostTree T;
    host_fit(host_topology_of(aee, n, builder), aee, n, T);  // (never false: the same array)
    return T;
}

// Topology of aee_topology, boxes of aee (rt_host_lbvh_refit). False for a finiteness mismatch.
inline bool host_refit(const float* aee_topology, const float* aee, uint32_t n, HostTree& T, uint32_t builder = 0u) {
    return host_fit(host_topology_of(aee_topology, n, builder), aee, n, T);
}

// The cost read-out on the host: every node slot, in any order (the sums are of integers).
inline void host_cost(const U4* hnodes, size_t node_slots, uint32_t root, uint64_t cost[4]) {
    for (int k = 0; k < 4; k++) cost[k] = 0;
    if ((root & LEAF_BIT) != 0u || (size_t)root >= node_slots) return;
    const double R = cost_root_area(hnodes[2 * (size_t)root], hnodes[2 * (size_t)root + 1]);
    for (size_t i = 0; i < node_slots; i++) cost_node(hnodes[2 * i], hnodes[2 * i + 1], R, cost);
}

}  // namespace hrt_lbvh
