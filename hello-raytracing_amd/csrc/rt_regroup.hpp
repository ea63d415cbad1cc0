// rt_regroup.hpp — what the host (renderer.cpp) and the device code (rt_regroup.hip) of rt_regroup_paths share: the
// mode 1 key as ONE inline function both compile (include/hrt.h rt_regroup has its definition in words), and the
// launcher's arguments. Built with -ffp-contract=off like everything else: the key's two f32 operations per axis stay two
// rounded operations, and no FMA is written here.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define HRT_REGROUP_FN __host__ __device__ inline
#else
#define HRT_REGROUP_FN inline
#endif

namespace hrt_regroup {

constexpr uint32_t KEY_MAX_CELL = 0x00FFFFFFu;  // mode 1: an index >= paths
constexpr uint32_t KEY_MAX_KEYS = 0xFFFFFFFFu;  // mode 2

HRT_REGROUP_FN uint32_t f32_bits(float x) {
    uint32_t u;
    __builtin_memcpy(&u, &x, sizeof u);
    return u;
}

// One axis of the cell: f = (o - lo) * inv as two rounded f32 operations; NaN and everything <= 0 give 0, f >= 128
// (+inf too) gives 127.
HRT_REGROUP_FN uint32_t cell_axis(float o, float lo, float inv) {
    const float e = o - lo;
    const float f = e * inv;
    if (!(f > 0.0f)) return 0u;
    if (f >= 128.0f) return 127u;
    return (uint32_t)f;
}

// Bit i of q (7 bits) to bit 3 i.
HRT_REGROUP_FN uint32_t spread3(uint32_t q) {
    uint32_t r = 0;
    for (uint32_t i = 0; i < 7u; i++) r |= ((q >> i) & 1u) << (3u * i);
    return r;
}

// The 24-bit key: the Morton code of the origin's cell in the 128^3 grid over the box in bits 3..23, the raw sign bits of
// d.x, d.y, d.z in bits 0, 1, 2. inv[k] = 128.0f / (hi[k] - lo[k]), divided on the host (box_inverse).
HRT_REGROUP_FN uint32_t cell_octant_key(const float o[3], const float d[3], const float lo[3], const float inv[3]) {
    const uint32_t qx = cell_axis(o[0], lo[0], inv[0]), qy = cell_axis(o[1], lo[1], inv[1]),
                   qz = cell_axis(o[2], lo[2], inv[2]);
    const uint32_t cell = spread3(qx) | (spread3(qy) << 1) | (spread3(qz) << 2);
    const uint32_t octant = (f32_bits(d[0]) >> 31) | ((f32_bits(d[1]) >> 31) << 1) | ((f32_bits(d[2]) >> 31) << 2);
    return (cell << 3) | octant;
}

// inv[k] = 128 / (hi[k] - lo[k]), host only (the IEEE division); false for a bad box: an extent that is NaN, infinite
// or below 2^-60 (zero and negative ones included), or an inverse that is not finite.
inline bool box_inverse(const float lo[3], const float hi[3], float inv[3]) {
    for (int k = 0; k < 3; k++) {
        const float ext = hi[k] - lo[k];
        if (!(ext >= 0x1p-60f) || !(ext <= 3.402823466e+38f)) return false;
        inv[k] = 128.0f / ext;
        if (!(inv[k] <= 3.402823466e+38f) || !(inv[k] >= -3.402823466e+38f)) return false;
    }
    return true;
}

// One rt_regroup_paths call, typed (hrt_launch_regroup). The scratch is the renderer's: `entries` holds 4 arrays of n
// u32 (key and index, twice: the passes ping-pong between them), `counts` holds 256 x ceil(n / RT_REGROUP_TILE) digit
// counts, then 4 x 256 digit totals (one set per pass, zeroed by the launcher), then the live count the key pass read.
struct Launch {
    const float* origins;
    const float* dirs;
    const uint32_t* keys;
    const uint32_t* index_in;
    const uint32_t* count_in;
    uint32_t* index_out;
    uint32_t* keys_out;
    uint32_t paths, mode;
    float lo[3], inv[3];
    uint32_t* entries;
    uint32_t* counts;
};
constexpr uint32_t TAIL_WORDS = 1040u;  // 4 x 256 digit totals + the live count (+ 15 unused)

}  // namespace hrt_regroup
