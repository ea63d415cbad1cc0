// rt_ploc.hip — the topology kernels of builder RT_TREE_PLOC (include/hrt.h rt_set_triangles_device_with): parallel
// locally-ordered clustering over the sorted Morton order, in place of k_lbvh_topology. A translation unit of its own: the
// code objects of rt_kernels.hip, rt_regroup.hip and rt_lbvh.hip do not move. Every rule is rt_lbvh.hpp's ("the PLOC
// topology"), shared with the host mirror host_topology_ploc: the tree is a pure function of the triangle array.
//
// hrt_launch_lbvh_ploc runs rt_lbvh.hip's front (prep, keys, sort), reads the finite count m' back, and then
//   k_ploc_init     one cluster per sorted position: its triangle's f64 box, the one-triangle leaf word; parent[0]
//   per iteration, while more than PLOC_TAIL clusters are left (the lists ping-pong in the fit's box slots, which the
//   fit writes before it reads; the keys and sorted keys, done with after the sort, hold the flags and the tile counts):
//     k_ploc_nn       one lane per cluster; the tile and 16 clusters on each side staged in LDS (the neighbour of a
//                     neighbour is needed); nn, the merge decision, the tile's survivors and pairs
//     k_ploc_scan     one workgroup: the exclusive sums of the tile counts; the totals to the status block
//     k_ploc_scatter  the next list, the node words, the parent links
//     (the host reads the cluster count back: it sizes the next grid and decides flat mode)
//   k_ploc_tail     one workgroup of 1024 lanes runs every remaining iteration in LDS
// and rt_lbvh.hip's fit. The only synchronisation between workgroups is the kernel boundary; inside a workgroup,
// __syncthreads. No lane waits, spins or polls on another workgroup, and no atomics are used.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrt.h"
#include "rt_lbvh.hpp"

hipError_t hrt_launch_lbvh_front(const hrt_lbvh::Launch& a, hipStream_t stream);  // rt_lbvh.hip
hipError_t hrt_launch_lbvh_fit(const hrt_lbvh::Launch& a, hipStream_t stream);    // rt_lbvh.hip

using hrt_lbvh::Cluster;
using hrt_lbvh::Launch;
using hrt_lbvh::U4;
constexpr uint32_t PLOC_WG = 256u;                   // lanes and clusters per tile of the per-iteration kernels
constexpr uint32_t PLOC_HALO = 2u * hrt_lbvh::PLOC_RADIUS;
constexpr uint32_t PLOC_STAGE = PLOC_WG + 2u * PLOC_HALO;
constexpr uint32_t TAIL_WG = hrt_lbvh::PLOC_TAIL;
static_assert(TAIL_WG == 1024u && PLOC_WG % 64u == 0u, "workgroups of whole waves; the tail is one full workgroup");

// state of a cluster after the merge decision, kept with its neighbour: state | nn << 2
constexpr uint32_t ST_ALONE = 0u, ST_LOWER = 1u, ST_DROPPED = 2u;

__global__ __launch_bounds__(256) void k_ploc_init(const Launch a, Cluster* __restrict__ out, uint32_t m) {
    const uint32_t p = blockIdx.x * PLOC_WG + threadIdx.x;
    if (p == 0u) a.parent[0] = hrt_lbvh::NO_PARENT;
    if (p >= m) return;
    const uint32_t j = a.order[p];  // (< n: the sort's permutation; checked all the same)
    if (j >= a.n) return;
    float aee[9];
    const float* const g = a.geo_out + 9u * (size_t)j;
#pragma unroll
    for (int k = 0; k < 9; k++) aee[k] = g[k];
    Cluster c;
    double cen[3];
    hrt_lbvh::tri_bounds(aee, c.lo, c.hi, cen);  // (true: the first m sorted positions are the finite ones)
    c.word = hrt_lbvh::LEAF_BIT | p << 4 | 1u;
    c.unused = 0u;
    out[p] = c;
}

// flags[i] = state | nn(i) << 2 for the c clusters of `in`; counts[2 b], [2 b + 1] = survivors and pairs of tile b.
__global__ __launch_bounds__(256) void k_ploc_nn(const Cluster* __restrict__ in, uint32_t c, uint32_t flat,
                                                 uint32_t* __restrict__ flags, uint32_t* __restrict__ counts) {
    __shared__ double s_box[6][PLOC_STAGE];
    __shared__ int s_nn[PLOC_WG + PLOC_HALO];
    __shared__ uint32_t s_cnt[PLOC_WG / 64u][2];
    const int base = (int)(blockIdx.x * PLOC_WG), g0 = base - (int)PLOC_HALO, ci = (int)c;
    for (int e = (int)threadIdx.x; e < (int)PLOC_STAGE; e += (int)PLOC_WG) {
        const int g = g0 + e;
        if (g >= 0 && g < ci) {
            const Cluster& q = in[g];
#pragma unroll
            for (int k = 0; k < 3; k++) {
                s_box[k][e] = q.lo[k];
                s_box[3 + k][e] = q.hi[k];
            }
        }
    }
    __syncthreads();
    // (cluster j of the window of a staged cluster is staged: |j - g| <= PLOC_RADIUS and g is PLOC_RADIUS inside the stage)
    const auto box = [&](int j, double lo[3], double hi[3]) {
        const int e = j - g0;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = s_box[k][e];
            hi[k] = s_box[3 + k][e];
        }
    };
    const int R = hrt_lbvh::PLOC_RADIUS;
    for (int e = R + (int)threadIdx.x; e < (int)PLOC_STAGE - R; e += (int)PLOC_WG) {
        const int g = g0 + e;
        if (g >= 0 && g < ci) s_nn[e - R] = hrt_lbvh::ploc_nearest(box, g, ci, flat != 0u);
    }
    __syncthreads();
    const int i = base + (int)threadIdx.x;
    bool survives = false, pairs = false;
    if (i < ci) {
        const int j = s_nn[i - g0 - R];  // (|j - i| <= PLOC_RADIUS: its nn is in s_nn too)
        const bool mutual = s_nn[j - g0 - R] == i;
        const uint32_t state = !mutual ? ST_ALONE : j > i ? ST_LOWER : ST_DROPPED;
        flags[i] = state | (uint32_t)j << 2;
        survives = state != ST_DROPPED;
        pairs = state == ST_LOWER;
    }
    // (every lane of the wave is here)
    const unsigned long long bs = __ballot(survives), bp = __ballot(pairs);
    if ((threadIdx.x & 63u) == 0u) {
        s_cnt[threadIdx.x >> 6][0] = (uint32_t)__popcll(bs);
        s_cnt[threadIdx.x >> 6][1] = (uint32_t)__popcll(bp);
    }
    __syncthreads();
    if (threadIdx.x < 2u) {
        uint32_t s = 0u;
        for (uint32_t w = 0; w < PLOC_WG / 64u; w++) s += s_cnt[w][threadIdx.x];
        counts[2u * blockIdx.x + threadIdx.x] = s;
    }
}

// The workgroup's exclusive sum of (x, y) over its lanes in lane order, and the totals. s_wave: one pair per wave.
template <uint32_t WAVES>
static __device__ inline void block_scan2(uint32_t& x, uint32_t& y, uint32_t& tx, uint32_t& ty, uint32_t (*s_wave)[2]) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t ix = x, iy = y;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t ux = __shfl_up(ix, off, 64), uy = __shfl_up(iy, off, 64);
        if (lane >= (uint32_t)off) {
            ix += ux;
            iy += uy;
        }
    }
    __syncthreads();  // (s_wave may still be read from the call before)
    if (lane == 63u) {
        s_wave[wave][0] = ix;
        s_wave[wave][1] = iy;
    }
    __syncthreads();
    uint32_t bx = 0u, by = 0u;
    tx = 0u;
    ty = 0u;
    for (uint32_t w = 0; w < WAVES; w++) {
        if (w == wave) {
            bx = tx;
            by = ty;
        }
        tx += s_wave[w][0];
        ty += s_wave[w][1];
    }
    x = bx + ix - x;
    y = by + iy - y;
}

// counts[2 b], [2 b + 1] become the survivors and pairs of the tiles before b; stat[10], [11] the totals.
__global__ __launch_bounds__(1024) void k_ploc_scan(uint32_t* __restrict__ counts, uint32_t tiles, uint64_t* __restrict__ stat) {
    __shared__ uint32_t s_wave[16][2];
    uint32_t run_s = 0u, run_p = 0u;
    for (uint32_t base = 0; base < tiles; base += 1024u) {  // (uniform: every lane takes every turn)
        const uint32_t b = base + threadIdx.x;
        uint32_t x = b < tiles ? counts[2u * b] : 0u, y = b < tiles ? counts[2u * b + 1u] : 0u, tx, ty;
        block_scan2<16>(x, y, tx, ty, s_wave);
        if (b < tiles) {
            counts[2u * b] = run_s + x;
            counts[2u * b + 1u] = run_p + y;
        }
        run_s += tx;
        run_p += ty;
    }
    if (threadIdx.x == 0u) {
        stat[10] = run_s;
        stat[11] = run_p;
    }
}

// One merge: node `id` over the clusters a (the lower position) and b; a becomes the merged cluster.
static __device__ inline void ploc_merge(Cluster& a, const Cluster& b, uint32_t id, U4* hnodes, uint32_t* parent, uint32_t n) {
    const uint32_t la = hrt_lbvh::ploc_link_slot(a.word, n), lb = hrt_lbvh::ploc_link_slot(b.word, n);
    if (id >= n - 1u || la >= 2u * n || lb >= 2u * n) return;  // (never: ids are below m' - 1 <= n - 1, positions below n)
    hnodes[2u * (size_t)id] = U4{0u, 0u, 0u, a.word};
    hnodes[2u * (size_t)id + 1u] = U4{0u, 0u, 0u, b.word};
    parent[la] = id << 1;
    parent[lb] = id << 1 | 1u;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        a.lo[k] = hrt_lbvh::dmin(a.lo[k], b.lo[k]);
        a.hi[k] = hrt_lbvh::dmax(a.hi[k], b.hi[k]);
    }
    a.word = id;
}

// next: the node ids not given out before this iteration. The s-th pair becomes node next - k + s.
__global__ __launch_bounds__(256) void k_ploc_scatter(const Cluster* __restrict__ in, Cluster* __restrict__ out, uint32_t c,
                                                      uint32_t next, const uint32_t* __restrict__ flags,
                                                      const uint32_t* __restrict__ counts, const uint64_t* __restrict__ stat,
                                                      U4* __restrict__ hnodes, uint32_t* __restrict__ parent, uint32_t n) {
    __shared__ uint32_t s_wave[PLOC_WG / 64u][2];
    const uint32_t i = blockIdx.x * PLOC_WG + threadIdx.x;
    const uint32_t f = i < c ? flags[i] : ST_DROPPED, state = f & 3u, j = f >> 2;
    const bool survives = state != ST_DROPPED, pairs = state == ST_LOWER;
    uint32_t rs = survives ? 1u : 0u, rp = pairs ? 1u : 0u, ts, tp;
    block_scan2<PLOC_WG / 64u>(rs, rp, ts, tp, s_wave);
    if (!survives) return;
    const uint32_t k = (uint32_t)stat[11], left = (uint32_t)stat[10];
    const uint32_t pos = counts[2u * blockIdx.x] + rs;
    if (pos >= left || left > c) return;  // (never)
    Cluster a = in[i];
    if (pairs) {
        const uint32_t s = counts[2u * blockIdx.x + 1u] + rp;
        if (j >= c || s >= k || k > next) return;  // (never)
        ploc_merge(a, in[j], next - k + s, hnodes, parent, n);
    }
    out[pos] = a;
}

// Every remaining iteration over c <= 1024 clusters, the list in LDS. t, next, flats: the state the iterations before left.
__global__ __launch_bounds__(1024) void k_ploc_tail(const Cluster* __restrict__ in, uint32_t c, uint32_t t, uint32_t next,
                                                    uint32_t flats, U4* __restrict__ hnodes, uint32_t* __restrict__ parent,
                                                    uint32_t n, uint64_t* __restrict__ stat) {
    __shared__ double s_box[6][TAIL_WG];
    __shared__ uint32_t s_word[TAIL_WG];
    __shared__ int s_nn[TAIL_WG];
    __shared__ uint32_t s_wave[TAIL_WG / 64u][2];
    const uint32_t tid = threadIdx.x;
    if (c > TAIL_WG) return;  // (never: the launcher's rule)
    if (tid < c) {
        const Cluster& q = in[tid];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            s_box[k][tid] = q.lo[k];
            s_box[3 + k][tid] = q.hi[k];
        }
        s_word[tid] = q.word;
    }
    __syncthreads();
    const auto box = [&](int j, double lo[3], double hi[3]) {
#pragma unroll
        for (int k = 0; k < 3; k++) {
            lo[k] = s_box[k][j];
            hi[k] = s_box[3 + k][j];
        }
    };
    // (c, t, next and flats are the same in every lane: the loop and its barriers are uniform)
    while (c >= 2u && t < hrt_lbvh::PLOC_LEVELS) {
        const bool flat = hrt_lbvh::ploc_flat(t, c);
        int j = 0;
        if (tid < c) {
            j = hrt_lbvh::ploc_nearest(box, (int)tid, (int)c, flat);
            s_nn[tid] = j;
        }
        __syncthreads();
        uint32_t state = ST_DROPPED;
        if (tid < c) state = s_nn[j] != (int)tid ? ST_ALONE : j > (int)tid ? ST_LOWER : ST_DROPPED;
        const bool survives = state != ST_DROPPED, pairs = state == ST_LOWER;
        uint32_t rs = survives ? 1u : 0u, rp = pairs ? 1u : 0u, left, k;
        block_scan2<TAIL_WG / 64u>(rs, rp, left, k, s_wave);
        Cluster a, b;
        if (survives) {
            box((int)tid, a.lo, a.hi);
            a.word = s_word[tid];
            a.unused = 0u;
            if (pairs) {
                box(j, b.lo, b.hi);
                b.word = s_word[j];
            }
        }
        __syncthreads();  // the old list has been read
        if (survives) {
            if (pairs && k <= next) ploc_merge(a, b, next - k + rp, hnodes, parent, n);
#pragma unroll
            for (int q = 0; q < 3; q++) {
                s_box[q][rs] = a.lo[q];
                s_box[3 + q][rs] = a.hi[q];
            }
            s_word[rs] = a.word;
        }
        __syncthreads();
        if (k == 0u || k > next) break;  // (never: a mutual pair exists, and the ids suffice)
        c = left;
        next -= k;
        t++;
        flats += flat ? 1u : 0u;
    }
    if (tid == 0u) {
        stat[10] = t;
        stat[11] = flats;
    }
}

// The whole build with builder 1. The staging and scratch buffers are the renderer's (rt_lbvh.hpp Launch); n > 0.
// pinned: STAT_WORDS u64 of pinned host memory for the read-backs. Synchronises the stream (after the sort, and once per
// iteration that takes its own launches); the fit is enqueued when it returns and the caller reads the status block.
hipError_t hrt_launch_lbvh_ploc(const Launch& a, uint64_t* pinned, hipStream_t stream) {
    const uint32_t n = a.n;
    if (n == 0) return hipSuccess;
    hipError_t e = hrt_launch_lbvh_front(a, stream);
    if (e == hipSuccess) e = hipMemcpyAsync(pinned, a.stat, hrt_lbvh::STAT_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) return e;
    const uint32_t m = (uint32_t)pinned[6];
    if (pinned[6] > n) return hipErrorUnknown;
    if (pinned[7] != 0u || m <= hrt_lbvh::LEAF_MAX) return hipSuccess;  // refused by the caller; or builder 0's tree without nodes
    Cluster* cur = (Cluster*)a.boxes;  // (2 n BOX_WORDS u64 = 128 n bytes: two lists of n 56-byte clusters)
    Cluster* other = cur + n;
    uint32_t* const flags = a.keys;          // n words, free after the sort
    uint32_t* const counts = a.keys_sorted;  // n words: two per tile of a list of more than PLOC_TAIL clusters
    hipLaunchKernelGGL(k_ploc_init, dim3((m + PLOC_WG - 1u) / PLOC_WG), dim3(PLOC_WG), 0, stream, a, cur, m);
    uint32_t c = m, next = m - 1u, t = 0u, flats = 0u;
    while (c > hrt_lbvh::PLOC_TAIL) {
        const uint32_t tiles = (c + PLOC_WG - 1u) / PLOC_WG;
        const bool flat = hrt_lbvh::ploc_flat(t, c);
        hipLaunchKernelGGL(k_ploc_nn, dim3(tiles), dim3(PLOC_WG), 0, stream, cur, c, flat ? 1u : 0u, flags, counts);
        hipLaunchKernelGGL(k_ploc_scan, dim3(1), dim3(1024), 0, stream, counts, tiles, a.stat);
        hipLaunchKernelGGL(k_ploc_scatter, dim3(tiles), dim3(PLOC_WG), 0, stream, cur, other, c, next, flags, counts, a.stat,
                           a.hnodes, a.parent, n);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(pinned + 10, a.stat + 10, 2 * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipStreamSynchronize(stream);
        if (e != hipSuccess) return e;
        const uint64_t left = pinned[10], k = pinned[11];
        // (a mutual pair exists, a pair leaves one cluster, and no more than half can go)
        if (k == 0u || left + k != c || k > next || left < (c + 1u) / 2u) return hipErrorUnknown;
        c = (uint32_t)left;
        next -= (uint32_t)k;
        t++;
        flats += flat ? 1u : 0u;
        Cluster* const x = cur;
        cur = other;
        other = x;
    }
    hipLaunchKernelGGL(k_ploc_tail, dim3(1), dim3(TAIL_WG), 0, stream, cur, c, t, next, flats, a.hnodes, a.parent, n, a.stat);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    return hrt_launch_lbvh_fit(a, stream);
}
