// rt_lbvh.hip — the kernels of rt_set_triangles_device (include/hrt.h): an LBVH over triangles the caller keeps in device
// memory, in the node format of the SAH triangle walk (rt_kernels.hip walk_sah). A translation unit of its own:
// rt_kernels.hip's code objects do not move. The rules are rt_lbvh.hpp's, shared with the host mirror.
//
// On the renderer's stream, one lane per triangle (or sorted position, or internal node) everywhere:
//   k_lbvh_prep      the TriDev and tri_geo records, the material check, the finite count, the root box
//   k_lbvh_keys      the Morton keys in the root box
//   (hrt_launch_regroup, mode 2: the stable sort of the keys; rt_regroup.hip)
//   k_lbvh_topology  Karras' node per lane: parent links, and the child words of the nodes the walk reads
//                    (builder RT_TREE_PLOC runs rt_ploc.hip's kernels in its place, between the same sort and fit)
//   k_lbvh_fit       the boxes, bottom up, packed
// The finite count m' is read on the device; every kernel is launched for the caller's n.
// Below them: rt_refit_triangles_device's two kernels (k_lbvh_refit_prep, k_lbvh_refit_fit: new boxes on the live tree's
// topology) and rt_get_tri_tree_cost's (k_tri_tree_cost).
//
// The fit is the one place where workgroups hand data to each other inside a launch. Every position's lane climbs; at a
// parent it leaves its f64 box in the slot of its side, then adds to the node's arrival counter; the first arriver stops,
// the second reads the other side's slot, packs the node and goes on with the union. No lane waits, spins or polls: a
// mistake here would give wrong boxes, never a hang. The XCDs' L2s and the CUs' L1s are not coherent, so the slot words
// are stored with agent-scope atomic stores (write-through), the storing wave waits for them (s_waitcnt vmcnt(0)) before
// its agent-scope counter add, and the second arriver reads the slot with agent-scope atomic loads (past the L1), issued
// after its add has returned. The counters are zeroed by the launcher on every call. Union of f64 boxes is exact and
// commutative: which child arrives first changes nothing.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrt.h"
#include "rt_device.hpp"
#include "rt_lbvh.hpp"
#include "rt_regroup.hpp"

hipError_t hrt_launch_regroup(const hrt_regroup::Launch& a, uint32_t n, hipStream_t stream);  // rt_regroup.hip

using hrt_lbvh::Launch;
using hrt_lbvh::U4;
constexpr uint32_t LBVH_WG = 256u;
#define HRT_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// The root box in the status block (rt_lbvh.hpp STAT_WORDS): the minima are kept as the maxima of the complemented keys,
// so that a zeroed block is the empty box.
static __device__ inline double root_lo(const uint64_t* stat, int k) { return hrt_lbvh::f64_from_key(~stat[k]); }
static __device__ inline double root_hi(const uint64_t* stat, int k) { return hrt_lbvh::f64_from_key(stat[3 + k]); }

static __device__ inline double wave_min(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = hrt_lbvh::dmin(x, __shfl_xor(x, off, 64));
    return x;
}
static __device__ inline double wave_max(double x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = hrt_lbvh::dmax(x, __shfl_xor(x, off, 64));
    return x;
}

__global__ __launch_bounds__(256) void k_lbvh_prep(const Launch a) {
    const uint32_t i = blockIdx.x * LBVH_WG + threadIdx.x;
    const bool valid = i < a.n;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, cen[3];
    bool finite = false, bad = false;
    if (valid) {
        const float4* const t = (const float4*)a.tris64 + 4u * (size_t)i;  // Triangle: a, b, c, (custom.xyz, material)
        const float4 va = t[0], vb = t[1], vc = t[2], vd = t[3];
        const float aee[9] = {va.x, va.y, va.z, vb.x - va.x, vb.y - va.y, vb.z - va.z, vc.x - va.x, vc.y - va.y, vc.z - va.z};
        float4* const o = (float4*)a.tris_out + 4u * (size_t)i;  // TriDev: a, e1, e2, (n.xyz, material)
        o[0] = float4{aee[0], aee[1], aee[2], 0.0f};
        o[1] = float4{aee[3], aee[4], aee[5], 0.0f};
        o[2] = float4{aee[6], aee[7], aee[8], 0.0f};
        o[3] = vd;
        float* const g = a.geo_out + 9u * (size_t)i;
#pragma unroll
        for (int k = 0; k < 9; k++) g[k] = aee[k];
        bad = __float_as_uint(vd.w) >= a.n_mats;
        finite = hrt_lbvh::tri_bounds(aee, lo, hi, cen);
        if (!finite)
            for (int k = 0; k < 3; k++) {
                lo[k] = INFINITY;
                hi[k] = -INFINITY;
            }
    }
    // (every lane of the wave is here: no lane has left)
    const unsigned long long nfin = __ballot(finite), nbad = __ballot(bad);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = wave_min(lo[k]);
        hi[k] = wave_max(hi[k]);
    }
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* const s = (unsigned long long*)a.stat;
        if (nfin != 0ull) {
            for (int k = 0; k < 3; k++) {
                __hip_atomic_fetch_max(&s[k], ~(unsigned long long)hrt_lbvh::f64_key(lo[k]), HRT_RLX_AGENT);
                __hip_atomic_fetch_max(&s[3 + k], (unsigned long long)hrt_lbvh::f64_key(hi[k]), HRT_RLX_AGENT);
            }
            __hip_atomic_fetch_add(&s[6], (unsigned long long)__popcll(nfin), HRT_RLX_AGENT);
        }
        if (nbad != 0ull) __hip_atomic_fetch_add(&s[7], (unsigned long long)__popcll(nbad), HRT_RLX_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_lbvh_keys(const Launch a) {
    const uint32_t i = blockIdx.x * LBVH_WG + threadIdx.x;
    if (i >= a.n) return;
    const float* const g = a.geo_out + 9u * (size_t)i;
    float aee[9];
#pragma unroll
    for (int k = 0; k < 9; k++) aee[k] = g[k];
    double lo[3], hi[3], cen[3];
    uint32_t key = hrt_lbvh::KEY_NONFINITE;
    if (hrt_lbvh::tri_bounds(aee, lo, hi, cen)) {
        double rlo[3], rhi[3];
        for (int k = 0; k < 3; k++) {
            rlo[k] = root_lo(a.stat, k);
            rhi[k] = root_hi(a.stat, k);
        }
        key = hrt_lbvh::morton_key(cen, rlo, rhi);
    }
    a.keys[i] = key;
}

__global__ __launch_bounds__(256) void k_lbvh_topology(const Launch a) {
    const uint32_t i = blockIdx.x * LBVH_WG + threadIdx.x;
    const uint32_t m = (uint32_t)a.stat[6];  // (<= n)
    if (i == 0u) a.parent[0] = hrt_lbvh::NO_PARENT;
    if (m <= hrt_lbvh::LEAF_MAX || i >= m - 1u) return;
    int first, last, split;
    hrt_lbvh::topology(a.keys_sorted, (int)m, (int)i, first, last, split);
    // (first <= split < last, all inside [0, m): the links below stay inside parent[0, 2 n))
    const uint32_t l = (uint32_t)split, r = l + 1u;
    a.parent[split == first ? a.n + l : l] = i << 1;
    a.parent[(int)r == last ? a.n + r : r] = i << 1 | 1u;
    if ((uint32_t)(last - first + 1) > hrt_lbvh::LEAF_MAX) {
        a.hnodes[2u * (size_t)i] = U4{0u, 0u, 0u, hrt_lbvh::child_word(first, split, split)};
        a.hnodes[2u * (size_t)i + 1u] = U4{0u, 0u, 0u, hrt_lbvh::child_word(split + 1, last, split + 1)};
    }
}

__global__ __launch_bounds__(256) void k_lbvh_fit(const Launch a) {
    const uint32_t p = blockIdx.x * LBVH_WG + threadIdx.x;
    const uint32_t m = (uint32_t)a.stat[6];
    if (m <= hrt_lbvh::LEAF_MAX || p >= m) return;
    float rc[3];
    for (int k = 0; k < 3; k++)
        rc[k] = hrt_lbvh::root_center(root_lo(a.stat, k), root_hi(a.stat, k));
    const uint32_t j = a.order[p];  // (< n: the sort's permutation; checked all the same)
    if (j >= a.n) return;
    float aee[9];
    {
        const float* const g = a.geo_out + 9u * (size_t)j;
#pragma unroll
        for (int k = 0; k < 9; k++) aee[k] = g[k];
    }
    double lo[3], hi[3], cen[3];
    if (!hrt_lbvh::tri_bounds(aee, lo, hi, cen)) return;  // (never: the first m sorted positions are the finite ones)
    uint32_t h = 0u, link = a.parent[a.n + p];
    // (at most 64 levels: a child's prefix is longer than its parent's, and delta < 64)
    for (uint32_t level = 0; level < 64u && link != hrt_lbvh::NO_PARENT; level++) {
        const uint32_t node = link >> 1, side = link & 1u;
        if (node >= m - 1u) return;  // (never: a link names an internal node)
        unsigned long long* const mine = (unsigned long long*)a.boxes + (2u * (size_t)node + side) * hrt_lbvh::BOX_WORDS;
        unsigned long long* const other = (unsigned long long*)a.boxes + (2u * (size_t)node + (side ^ 1u)) * hrt_lbvh::BOX_WORDS;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            __hip_atomic_store(&mine[k], (unsigned long long)hrt_lbvh::f64_bits(lo[k]), HRT_RLX_AGENT);
            __hip_atomic_store(&mine[3 + k], (unsigned long long)hrt_lbvh::f64_bits(hi[k]), HRT_RLX_AGENT);
        }
        __hip_atomic_store(&mine[6], (unsigned long long)h, HRT_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slot's stores are complete before the arrival counts
        const uint32_t before = __hip_atomic_fetch_add(&a.arrivals[node], 1u, HRT_RLX_AGENT);
        asm volatile("" ::: "memory");  // (the slot loads below stay below the add)
        if (before == 0u) return;       // the first arriver: the sibling will take this box along
        double olo[3], ohi[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            olo[k] = hrt_lbvh::f64_from_bits(__hip_atomic_load(&other[k], HRT_RLX_AGENT));
            ohi[k] = hrt_lbvh::f64_from_bits(__hip_atomic_load(&other[3 + k], HRT_RLX_AGENT));
        }
        const uint32_t oh = (uint32_t)__hip_atomic_load(&other[6], HRT_RLX_AGENT);
        // (written by k_lbvh_topology, an earlier launch; this lane alone rewrites the node)
        const uint32_t lw = a.hnodes[2u * (size_t)node].w, rw = a.hnodes[2u * (size_t)node + 1u].w;
        if (lw != 0u) {  // a node the walk reads
            a.hnodes[2u * (size_t)node] = side == 0u ? hrt_lbvh::pack_child(lo, hi, rc, lw) : hrt_lbvh::pack_child(olo, ohi, rc, lw);
            a.hnodes[2u * (size_t)node + 1u] = side == 0u ? hrt_lbvh::pack_child(olo, ohi, rc, rw) : hrt_lbvh::pack_child(lo, hi, rc, rw);
            h = 1u + max(h, oh);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = hrt_lbvh::dmin(lo[k], olo[k]);
            hi[k] = hrt_lbvh::dmax(hi[k], ohi[k]);
        }
        if (node == 0u) a.stat[8] = h;
        link = a.parent[node];
    }
}

// Host-side launcher: the staging and scratch buffers are the renderer's (rt_lbvh.hpp Launch has the sizes). n > 0.
// In three parts, because the PLOC builder (rt_ploc.hip) runs the first and the last around a topology of its own.
// Everything up to the sort: the zeroing, the prep, the keys, the stable sort.
hipError_t hrt_launch_lbvh_front(const Launch& a, hipStream_t stream) {
    const uint32_t n = a.n;
    if (n == 0) return hipSuccess;
    hipError_t e = hipMemsetAsync(a.stat, 0, hrt_lbvh::STAT_WORDS * sizeof(uint64_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.arrivals, 0, (size_t)n * sizeof(uint32_t), stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.hnodes, 0, 2u * (size_t)(n > 1u ? n - 1u : 1u) * sizeof(U4), stream);
    if (e != hipSuccess) return e;
    const dim3 block(LBVH_WG), grid((n + LBVH_WG - 1u) / LBVH_WG);
    hipLaunchKernelGGL(k_lbvh_prep, grid, block, 0, stream, a);
    hipLaunchKernelGGL(k_lbvh_keys, grid, block, 0, stream, a);
    hrt_regroup::Launch s{};
    s.keys = a.keys;
    s.index_out = a.order;
    s.keys_out = a.keys_sorted;
    s.paths = n;
    s.mode = RT_REGROUP_KEYS;
    s.entries = a.sort_entries;
    s.counts = a.sort_counts;
    return hrt_launch_regroup(s, n, stream);
}

// The fit over whatever topology the parent links and child words hold.
hipError_t hrt_launch_lbvh_fit(const Launch& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_lbvh_fit, dim3((a.n + LBVH_WG - 1u) / LBVH_WG), dim3(LBVH_WG), 0, stream, a);
    return hipGetLastError();
}

// Builder 0: Karras' topology between the two.
hipError_t hrt_launch_lbvh(const Launch& a, hipStream_t stream) {
    const uint32_t n = a.n;
    if (n == 0) return hipSuccess;
    const hipError_t e = hrt_launch_lbvh_front(a, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_lbvh_topology, dim3((n + LBVH_WG - 1u) / LBVH_WG), dim3(LBVH_WG), 0, stream, a);
    return hrt_launch_lbvh_fit(a, stream);
}

// ---- rt_refit_triangles_device: the boxes of a moved mesh on the live tree's topology ----
// Two kernels of their own (the four above and their by-value Launch stay as they are): no keys, no sort, no topology.
//   k_lbvh_refit_prep  k_lbvh_prep's work into the staging records, a count of the triangles whose finiteness is not
//                      the live tri_geo's (stat[9]), and the zeroing the fit needs (arrival counters, staging nodes)
//   k_lbvh_refit_fit   k_lbvh_fit's climb over the live order and parent links; the child words come from the live node
//                      array (read only in this launch) and the packed nodes go to the staging one
// The hand-off is k_lbvh_fit's, word for word: agent-scope atomic stores of the slot, s_waitcnt vmcnt(0), the agent-scope
// arrival add, agent-scope atomic loads of the sibling's slot after the add has returned. No lane waits, spins or polls.
using hrt_lbvh::Refit;

__global__ __launch_bounds__(256) void k_lbvh_refit_prep(const Refit a) {
    const uint32_t i = blockIdx.x * LBVH_WG + threadIdx.x;
    const bool valid = i < a.n;
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, cen[3];
    bool finite = false, bad = false, changed = false;
    if (valid) {
        const float4* const t = (const float4*)a.tris64 + 4u * (size_t)i;  // Triangle: a, b, c, (custom.xyz, material)
        const float4 va = t[0], vb = t[1], vc = t[2], vd = t[3];
        const float aee[9] = {va.x, va.y, va.z, vb.x - va.x, vb.y - va.y, vb.z - va.z, vc.x - va.x, vc.y - va.y, vc.z - va.z};
        float4* const o = (float4*)a.tris_out + 4u * (size_t)i;  // TriDev: a, e1, e2, (n.xyz, material)
        o[0] = float4{aee[0], aee[1], aee[2], 0.0f};
        o[1] = float4{aee[3], aee[4], aee[5], 0.0f};
        o[2] = float4{aee[6], aee[7], aee[8], 0.0f};
        o[3] = vd;
        float* const g = a.geo_out + 9u * (size_t)i;
        const float* const live = a.geo_live + 9u * (size_t)i;
        bool was = true;
#pragma unroll
        for (int k = 0; k < 9; k++) {
            g[k] = aee[k];
            was = was && hrt_lbvh::f32_finite(live[k]);
        }
        bad = __float_as_uint(vd.w) >= a.n_mats;
        finite = hrt_lbvh::tri_bounds(aee, lo, hi, cen);
        changed = finite != was;
        if (!finite)
            for (int k = 0; k < 3; k++) {
                lo[k] = INFINITY;
                hi[k] = -INFINITY;
            }
        // node slot i of the fit that follows (m - 1 <= n - 1 slots): its arrival counter, and the staging node, which may
        // hold an older, different tree: a slot no child word names stays zero
        if (a.m > hrt_lbvh::LEAF_MAX && i < a.m - 1u) {
            a.arrivals[i] = 0u;
            a.hnodes[2u * (size_t)i] = U4{0u, 0u, 0u, 0u};
            a.hnodes[2u * (size_t)i + 1u] = U4{0u, 0u, 0u, 0u};
        }
    }
    // (every lane of the wave is here: no lane has left)
    const unsigned long long nfin = __ballot(finite), nbad = __ballot(bad), nchg = __ballot(changed);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        lo[k] = wave_min(lo[k]);
        hi[k] = wave_max(hi[k]);
    }
    if ((threadIdx.x & 63u) == 0u) {
        unsigned long long* const s = (unsigned long long*)a.stat;
        if (nfin != 0ull) {
            for (int k = 0; k < 3; k++) {
                __hip_atomic_fetch_max(&s[k], ~(unsigned long long)hrt_lbvh::f64_key(lo[k]), HRT_RLX_AGENT);
                __hip_atomic_fetch_max(&s[3 + k], (unsigned long long)hrt_lbvh::f64_key(hi[k]), HRT_RLX_AGENT);
            }
            __hip_atomic_fetch_add(&s[6], (unsigned long long)__popcll(nfin), HRT_RLX_AGENT);
        }
        if (nbad != 0ull) __hip_atomic_fetch_add(&s[7], (unsigned long long)__popcll(nbad), HRT_RLX_AGENT);
        if (nchg != 0ull) __hip_atomic_fetch_add(&s[9], (unsigned long long)__popcll(nchg), HRT_RLX_AGENT);
    }
}

__global__ __launch_bounds__(256) void k_lbvh_refit_fit(const Refit a) {
    const uint32_t p = blockIdx.x * LBVH_WG + threadIdx.x;
    const uint32_t m = a.m;  // (<= n: the launcher checks)
    if (m <= hrt_lbvh::LEAF_MAX || p >= m) return;
    float rc[3];
    for (int k = 0; k < 3; k++)
        rc[k] = hrt_lbvh::root_center(root_lo(a.stat, k), root_hi(a.stat, k));
    const uint32_t j = a.order[p];  // (< n: the live tree's permutation; checked all the same)
    if (j >= a.n) return;
    float aee[9];
    {
        const float* const g = a.geo_out + 9u * (size_t)j;
#pragma unroll
        for (int k = 0; k < 9; k++) aee[k] = g[k];
    }
    double lo[3], hi[3], cen[3];
    // (a position's triangle that is not finite: the prep has counted it in stat[9] and the host refuses the result)
    if (!hrt_lbvh::tri_bounds(aee, lo, hi, cen)) return;
    uint32_t h = 0u, link = a.parent[a.n + p];
    for (uint32_t level = 0; level < 64u && link != hrt_lbvh::NO_PARENT; level++) {
        const uint32_t node = link >> 1, side = link & 1u;
        if (node >= m - 1u) return;  // (never: a link names an internal node)
        unsigned long long* const mine = (unsigned long long*)a.boxes + (2u * (size_t)node + side) * hrt_lbvh::BOX_WORDS;
        unsigned long long* const other = (unsigned long long*)a.boxes + (2u * (size_t)node + (side ^ 1u)) * hrt_lbvh::BOX_WORDS;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            __hip_atomic_store(&mine[k], (unsigned long long)hrt_lbvh::f64_bits(lo[k]), HRT_RLX_AGENT);
            __hip_atomic_store(&mine[3 + k], (unsigned long long)hrt_lbvh::f64_bits(hi[k]), HRT_RLX_AGENT);
        }
        __hip_atomic_store(&mine[6], (unsigned long long)h, HRT_RLX_AGENT);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the slot's stores are complete before the arrival counts
        const uint32_t before = __hip_atomic_fetch_add(&a.arrivals[node], 1u, HRT_RLX_AGENT);
        asm volatile("" ::: "memory");  // (the slot loads below stay below the add)
        if (before == 0u) return;       // the first arriver: the sibling will take this box along
        double olo[3], ohi[3];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            olo[k] = hrt_lbvh::f64_from_bits(__hip_atomic_load(&other[k], HRT_RLX_AGENT));
            ohi[k] = hrt_lbvh::f64_from_bits(__hip_atomic_load(&other[3 + k], HRT_RLX_AGENT));
        }
        const uint32_t oh = (uint32_t)__hip_atomic_load(&other[6], HRT_RLX_AGENT);
        // (the live array: written by an earlier call; this lane alone writes the staging node)
        const uint32_t lw = a.hnodes_live[2u * (size_t)node].w, rw = a.hnodes_live[2u * (size_t)node + 1u].w;
        if (lw != 0u) {  // a node the walk reads
            a.hnodes[2u * (size_t)node] = side == 0u ? hrt_lbvh::pack_child(lo, hi, rc, lw) : hrt_lbvh::pack_child(olo, ohi, rc, lw);
            a.hnodes[2u * (size_t)node + 1u] = side == 0u ? hrt_lbvh::pack_child(olo, ohi, rc, rw) : hrt_lbvh::pack_child(lo, hi, rc, rw);
            h = 1u + max(h, oh);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = hrt_lbvh::dmin(lo[k], olo[k]);
            hi[k] = hrt_lbvh::dmax(hi[k], ohi[k]);
        }
        if (node == 0u) a.stat[8] = h;
        link = a.parent[node];
    }
}

// n > 0, m <= n. One memset (the status block: the prep's atomics start from it), the prep, the fit. The prep also
// zeroes the fit's arrival counters and the staging node slots of the live tree.
hipError_t hrt_launch_lbvh_refit(const Refit& a, hipStream_t stream) {
    const uint32_t n = a.n;
    if (n == 0 || a.m > n) return n == 0 ? hipSuccess : hipErrorInvalidValue;
    const uint32_t slots = hrt_lbvh::node_slots(a.m);
    hipError_t e = hipMemsetAsync(a.stat, 0, hrt_lbvh::STAT_WORDS * sizeof(uint64_t), stream);
    if (e != hipSuccess) return e;
    const dim3 block(LBVH_WG);
    hipLaunchKernelGGL(k_lbvh_refit_prep, dim3((n + LBVH_WG - 1u) / LBVH_WG), block, 0, stream, a);
    if (slots) hipLaunchKernelGGL(k_lbvh_refit_fit, dim3((a.m + LBVH_WG - 1u) / LBVH_WG), block, 0, stream, a);
    return hipGetLastError();
}

// ---- rt_get_tri_tree_cost: hrt_lbvh::cost_node over every node slot of a tree in the tri_bvh = 1 node format ----
// One lane per slot; the four words are summed per wave and added once per wave and word (integers: any order).
static __device__ inline unsigned long long wave_sum(unsigned long long x) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

__global__ __launch_bounds__(256) void k_tri_tree_cost(const U4* __restrict__ hnodes, uint32_t slots, uint32_t root,
                                                       unsigned long long* __restrict__ out) {
    const uint32_t i = blockIdx.x * LBVH_WG + threadIdx.x;
    uint64_t c[4] = {0u, 0u, 0u, 0u};
    if (i < slots && root < slots) {
        const double R = hrt_lbvh::cost_root_area(hnodes[2u * (size_t)root], hnodes[2u * (size_t)root + 1u]);
        hrt_lbvh::cost_node(hnodes[2u * (size_t)i], hnodes[2u * (size_t)i + 1u], R, c);
    }
    // (every lane of the wave is here)
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long s = wave_sum((unsigned long long)c[k]);
        if ((threadIdx.x & 63u) == 0u && s != 0ull) __hip_atomic_fetch_add(&out[k], s, HRT_RLX_AGENT);
    }
}

// out: 4 u64 in device memory, zeroed here. root: a node index (the caller answers a leaf root word itself).
hipError_t hrt_launch_tri_tree_cost(const void* hnodes, uint32_t slots, uint32_t root, uint64_t* out, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out, 0, 4u * sizeof(uint64_t), stream);
    if (e != hipSuccess || slots == 0u || root >= slots) return e;
    hipLaunchKernelGGL(k_tri_tree_cost, dim3((slots + LBVH_WG - 1u) / LBVH_WG), dim3(LBVH_WG), 0, stream, (const U4*)hnodes, slots,
                       root, (unsigned long long*)out);
    return hipGetLastError();
}
