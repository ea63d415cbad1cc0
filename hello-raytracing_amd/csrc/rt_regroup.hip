// rt_regroup.hip — the kernels of rt_regroup_paths (include/hrt.h rt_regroup): a key pass, then a stable
// least-significant-digit radix sort of (key, path index) pairs over 8-bit digits, three kernels per pass on the
// renderer's stream: count, scan, scatter. A translation unit of its own: rt_kernels.hip's code objects do not move.
//
// Shape. One entry per lane everywhere. The count and scatter kernels give each 256-lane workgroup one TILE of
// RT_REGROUP_TILE = 1024 consecutive entries, as 16 runs of 64: in round k = 0..3 wave w takes run 4 k + w, so a round
// reads 256 consecutive entries. Every kernel is launched for the host's n and reads the live count on the device (the
// key pass reads *count_in as k_bounce_rays does and leaves min(n, *count_in) in the scratch for the sort's kernels, so a
// sort never sees two values of it); lanes and workgroups past the live count leave after reading it.
//
// Stability. The digit counts are laid out digit-major, counts[digit * tiles + tile], so their exclusive scan in that
// order gives each (digit, tile) the first output position of the tile's entries with that digit: smaller digits first,
// and within a digit the tiles in input order. Inside a tile the 16 runs are ordered the same way: a lane's rank among the
// lanes of its run (= its wave, in that round) with the same digit comes from eight __ballots, one per digit bit, and
// mbcnt of the matching mask; the run's count per digit goes to LDS, and lane d of the workgroup turns the 16 counts of
// digit d into the runs' offsets. Nothing depends on which lane or wave gets somewhere first (an LDS atomic rank would).
//
// No workgroup waits for another: the stream order between the kernels is the only dependence. The digit totals the scan
// starts from are summed with relaxed agent-scope integer atomics by the count kernel (a sum does not depend on the
// order of its terms) and read by the next kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hrt.h"
#include "rt_regroup.hpp"

// (the kernels are named at file scope, as in rt_kernels.hip: profilers and scripts/resource_usage.py print the plain names)
constexpr uint32_t TILE = RT_REGROUP_TILE;
constexpr uint32_t WG = 256u;             // lanes per workgroup: 4 waves
constexpr uint32_t ROUNDS = TILE / WG;    // 4
constexpr uint32_t RUNS = TILE / 64u;     // 16
static_assert(TILE % WG == 0 && ROUNDS * 4u == RUNS, "a tile is whole rounds of four 64-entry runs");

static __device__ inline uint32_t tiles_of(uint32_t live) { return (live + TILE - 1u) / TILE; }

// The lanes of this wave that are valid and hold the same 8-bit digit as this lane: eight ballots, one per digit bit.
// Called by every lane of the wave (no lane has left); an invalid lane's result is not used.
static __device__ inline unsigned long long match_digit(uint32_t digit, bool valid) {
    unsigned long long m = __ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < 8u; b++) {
        const bool bit = ((digit >> b) & 1u) != 0u;
        const unsigned long long v = __ballot(valid && bit);
        m &= bit ? v : ~v;
    }
    return m;
}

static __device__ inline uint32_t lanes_below(unsigned long long m) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// Inclusive sum over the wave's 64 lanes.
static __device__ inline uint32_t wave_inclusive(uint32_t x) {
    const uint32_t lane = threadIdx.x & 63u;
#pragma unroll
    for (uint32_t off = 1u; off < 64u; off <<= 1) {
        const uint32_t y = (uint32_t)__shfl_up((int)x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// The key pass: entry i < live is path j = index_in ? index_in[i] : i; (key, j) go to the sort's first buffer. Every
// read of index_in happens here, before any kernel writes index_out: that makes index_out == index_in safe.
template <uint32_t MODE>
__global__ __launch_bounds__(256) void k_regroup_keys(const hrt_regroup::Launch a, uint32_t n, uint32_t* __restrict__ key_out,
                                                      uint32_t* __restrict__ idx_out, uint32_t* __restrict__ live_out) {
    const uint32_t i = blockIdx.x * WG + threadIdx.x;
    uint32_t live = n;
    if (a.count_in != nullptr) live = min(n, *a.count_in);
    if (i == 0u) *live_out = live;  // (n > 0: lane 0 of workgroup 0 exists)
    if (i >= live) return;
    const uint32_t j = a.index_in != nullptr ? a.index_in[i] : i;
    uint32_t key = MODE == RT_REGROUP_CELL_OCTANT ? hrt_regroup::KEY_MAX_CELL : hrt_regroup::KEY_MAX_KEYS;
    if (j < a.paths) {  // (nothing is read through an index >= paths)
        if (MODE == RT_REGROUP_CELL_OCTANT) {
            const float* const po = a.origins + (size_t)j * 3u;
            const float* const pd = a.dirs + (size_t)j * 3u;
            const float o[3] = {po[0], po[1], po[2]}, d[3] = {pd[0], pd[1], pd[2]};
            key = hrt_regroup::cell_octant_key(o, d, a.lo, a.inv);
        } else {
            key = a.keys[j];
        }
    }
    key_out[i] = key;
    idx_out[i] = j;
}

// Count: the tile's entries per digit, to counts[digit * tiles + tile], and added to the pass's digit totals.
__global__ __launch_bounds__(256) void k_regroup_count(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ live_p,
                                                       uint32_t shift, uint32_t* __restrict__ counts,
                                                       uint32_t* __restrict__ totals) {
    __shared__ uint32_t hist[256];
    const uint32_t live = *live_p;
    const uint32_t base = blockIdx.x * TILE;
    if (base >= live) return;  // (the whole workgroup)
    const uint32_t tiles = tiles_of(live);
    hist[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t i = base + k * WG + threadIdx.x;
        const bool valid = i < live;
        const uint32_t digit = valid ? (keys[i] >> shift) & 255u : 0u;
        const unsigned long long m = match_digit(digit, valid);
        if (valid && lanes_below(m) == 0u) atomicAdd(&hist[digit], (uint32_t)__popcll(m));  // (one lane per digit and wave)
    }
    __syncthreads();
    const uint32_t c = hist[threadIdx.x];
    counts[threadIdx.x * tiles + blockIdx.x] = c;
    if (c != 0u) __hip_atomic_fetch_add(&totals[threadIdx.x], c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Scan: workgroup d turns row d of the counts (the tiles' counts of digit d) into output positions, in place: the
// entries of all smaller digits (the totals below d) plus the exclusive sum along the row, 256 tiles per iteration.
__global__ __launch_bounds__(256) void k_regroup_scan(const uint32_t* __restrict__ live_p, uint32_t* __restrict__ counts,
                                                      const uint32_t* __restrict__ totals) {
    __shared__ uint32_t wsum[4];
    const uint32_t live = *live_p;
    if (live == 0u) return;
    const uint32_t tiles = tiles_of(live);
    const uint32_t d = blockIdx.x, t = threadIdx.x, w = t >> 6, lane = t & 63u;
    // the entries of the digits below d
    uint32_t x = t < d ? totals[t] : 0u;
    x = wave_inclusive(x);
    if (lane == 63u) wsum[w] = x;
    __syncthreads();
    uint32_t carry = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    __syncthreads();
    uint32_t* const row = counts + (size_t)d * tiles;
    for (uint32_t c0 = 0; c0 < tiles; c0 += WG) {  // (uniform: every lane takes every iteration and both barriers)
        const uint32_t i = c0 + t;
        const uint32_t v = i < tiles ? row[i] : 0u;
        const uint32_t incl = wave_inclusive(v);
        if (lane == 63u) wsum[w] = incl;
        __syncthreads();
        uint32_t before = 0u;
        if (w > 0u) before += wsum[0];
        if (w > 1u) before += wsum[1];
        if (w > 2u) before += wsum[2];
        const uint32_t all = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (i < tiles) row[i] = carry + before + (incl - v);
        carry += all;
        __syncthreads();  // (wsum is rewritten by the next iteration)
    }
}

// Scatter: each entry of the tile to (its digit's position for this tile) + (the entries of the tile's earlier runs with
// that digit) + (its rank among its own run's lanes with that digit). The last pass writes the caller's buffers.
__global__ __launch_bounds__(256) void k_regroup_scatter(const uint32_t* __restrict__ keys_in, const uint32_t* __restrict__ idx_in,
                                                         const uint32_t* __restrict__ live_p, uint32_t shift,
                                                         const uint32_t* __restrict__ offsets, uint32_t* keys_out,
                                                         uint32_t* idx_out) {
    __shared__ uint32_t run_ofs[RUNS][256];  // [run][digit]: the run's count, then its first output position
    const uint32_t live = *live_p;
    const uint32_t base = blockIdx.x * TILE;
    if (base >= live) return;  // (the whole workgroup)
    const uint32_t tiles = tiles_of(live);
    const uint32_t t = threadIdx.x, w = t >> 6;
#pragma unroll
    for (uint32_t r = 0; r < RUNS; r++) run_ofs[r][t] = 0u;
    __syncthreads();
    uint32_t key[ROUNDS], idx[ROUNDS], rank[ROUNDS];
#pragma unroll
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t i = base + k * WG + t;
        const bool valid = i < live;
        key[k] = valid ? keys_in[i] : 0u;
        idx[k] = valid ? idx_in[i] : 0u;
        const uint32_t digit = (key[k] >> shift) & 255u;
        const unsigned long long m = match_digit(digit, valid);
        rank[k] = lanes_below(m);
        if (valid && rank[k] == 0u) run_ofs[k * 4u + w][digit] = (uint32_t)__popcll(m);  // (one lane per digit and run)
    }
    __syncthreads();
    {  // lane t owns digit t: the runs' counts become their positions, run 0 first
        uint32_t o = offsets[t * tiles + blockIdx.x];
#pragma unroll
        for (uint32_t r = 0; r < RUNS; r++) {
            const uint32_t c = run_ofs[r][t];
            run_ofs[r][t] = o;
            o += c;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t k = 0; k < ROUNDS; k++) {
        const uint32_t i = base + k * WG + t;
        if (i < live) {
            const uint32_t dst = run_ofs[k * 4u + w][(key[k] >> shift) & 255u] + rank[k];
            if (dst < live) {  // (always, for counts and offsets of these keys: the store stays inside [0, live) regardless)
                idx_out[dst] = idx[k];
                if (keys_out != nullptr) keys_out[dst] = key[k];
            }
        }
    }
}

// Host-side launcher of rt_regroup_paths: the key pass for ceil(n / 256) workgroups, then per pass count and scatter for
// ceil(n / TILE) workgroups and the scan for 256. The passes ping-pong between the scratch's two (key, index) buffers;
// the last one writes index_out / keys_out.
hipError_t hrt_launch_regroup(const hrt_regroup::Launch& a, uint32_t n, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint32_t tiles = (n + TILE - 1u) / TILE;
    uint32_t* const key_buf[2] = {a.entries, a.entries + 2u * (size_t)n};
    uint32_t* const idx_buf[2] = {a.entries + (size_t)n, a.entries + 3u * (size_t)n};
    uint32_t* const totals = a.counts + 256u * (size_t)tiles;
    uint32_t* const live = totals + 4u * 256u;
    hipError_t e = hipMemsetAsync(totals, 0, 4u * 256u * sizeof(uint32_t), stream);
    if (e != hipSuccess) return e;
    const dim3 block(WG), grid_keys((n + WG - 1u) / WG), grid_tiles(tiles), grid_scan(256);
    const uint32_t passes = a.mode == RT_REGROUP_CELL_OCTANT ? 3u : 4u;
    if (a.mode == RT_REGROUP_CELL_OCTANT)
        hipLaunchKernelGGL((k_regroup_keys<RT_REGROUP_CELL_OCTANT>), grid_keys, block, 0, stream, a, n, key_buf[0], idx_buf[0],
                           live);
    else
        hipLaunchKernelGGL((k_regroup_keys<RT_REGROUP_KEYS>), grid_keys, block, 0, stream, a, n, key_buf[0], idx_buf[0], live);
    for (uint32_t p = 0; p < passes; p++) {
        const uint32_t src = p & 1u, dst = src ^ 1u;
        const bool last = p + 1u == passes;
        hipLaunchKernelGGL(k_regroup_count, grid_tiles, block, 0, stream, key_buf[src], live, 8u * p, a.counts,
                           totals + 256u * p);
        hipLaunchKernelGGL(k_regroup_scan, grid_scan, block, 0, stream, live, a.counts, totals + 256u * p);
        hipLaunchKernelGGL(k_regroup_scatter, grid_tiles, block, 0, stream, key_buf[src], idx_buf[src], live, 8u * p, a.counts,
                           last ? a.keys_out : key_buf[dst], last ? a.index_out : idx_buf[dst]);
    }
    return hipGetLastError();
}
