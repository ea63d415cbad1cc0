/*
 * hrt_testing.h — test-only entry points of libhrt.so (fault injection). Not part of the drop-in surface
 * (include/hrt.h): the reference has nothing to bind here, and a product caller never needs
 * them. The parity suite uses them to drive the sample queue's rare paths on a healthy device.
 */
#ifndef HRT_TESTING_H
#define HRT_TESTING_H

#include "hrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ring_slots_max: the fold ring gets at most this many job slots (rounded down to a power of two; 0 = no cap),
 *   so that nearly every job waits for one.
 * fail_alloc_above_mb: colour-fold allocations above this many MiB fail as a refused hipMalloc would (0 = off);
 *   the draw then shrinks them.
 * Both stay set until changed; a new renderer starts with both 0. */
int rt_testing_set_faults(rt_renderer *r, uint32_t ring_slots_max, uint32_t fail_alloc_above_mb);

/* hold: the descent hold of the sphere program's suspendable-walk kernel with LDS nodes (k_trace_split): after a box
 *   step that fewer than `hold` lanes of a wave would follow with another one, while other walking lanes wait at a
 *   leaf or a miss, the wave leaves the descent and the stragglers take their next step with the lanes that popped.
 *   0..64 (RT_ERR_ARG above), 0 = off. Every value draws the same image with the same test counts; only the speed
 *   changes. Stays set until changed; a new renderer starts with the measured default. */
int rt_testing_set_descent_hold(rt_renderer *r, uint32_t hold);

/* rays_per_lane: R of rt_trace_rays' kernel (k_radiance_rays): a wave owns 64 R consecutive rays and each lane traces
 *   R of them one after another. 0..64 (RT_ERR_ARG above), 0 = the host's rule by batch size. Every value gives the
 *   same radiance and queries; only the speed changes (scripts/bench_trace_rays.py sweeps it). Stays set until changed;
 *   a new renderer starts with 0. */
int rt_testing_set_trace_rays_per_lane(rt_renderer *r, uint32_t rays_per_lane);

/* The leaves of the sphere culling BVH the renderer would build over n_slots slots (centers_radii: cx, cy, cz, radius per
 *   slot, padding slots as zeros). Host only, no device.
 * leaves: one word per leaf in BVH order, first << 4 | count (first: the leaf's first position in BVH order).
 * slots: the slot of every BVH position, then the slots of the large list (scanned for every ray, not in the tree).
 * counts: {leaves, BVH positions, large-list entries, tree depth}; always written. With both capacities 0 only the
 *   counts are returned; a capacity that is too small otherwise is RT_ERR_ARG. */
int rt_testing_sphere_bvh_leaves(const float *centers_radii, uint32_t n_slots, uint32_t *leaves, uint32_t leaf_cap,
                                 int32_t *slots, uint32_t slot_cap, uint32_t counts[4]);

/* Blocking read-back of the triangle tree the renderer walks with tri_bvh = 1 or with device geometry, in the format
 *   and with the capacity rules of rt_host_lbvh_build (info[1] = info[2] = the leaf positions). A host SAH tree that
 *   was not built yet (rt_set_bvh, no tri_bvh = 1 query so far) is built first. RT_ERR_ARG in the sphere program. */
int rt_testing_get_tri_tree(rt_renderer *r, void *hnodes_out, size_t hnode_cap, uint32_t *order_out, size_t order_cap,
                            uint32_t info[8], float root[4]);

/* Blocking read-back of what cost-ordered dealing (rt_params.cost_order) has learnt: per tile (8x8 pixels, raster order
 *   over the renderer's rows) the sum of its pixels' cost counters from the last learning launch — a finished sample adds
 *   its bounces + 1 to its pixel — and the tile order built from the sums, a permutation of the tiles. count: the tiles
 *   the renderer holds an order for (0 before the first learning launch), always written. With cap 0 only the count is
 *   returned; a smaller cap otherwise is RT_ERR_ARG. */
int rt_testing_get_tile_order(rt_renderer *r, uint32_t *sum_out, uint32_t *order_out, size_t cap, size_t *count);

#ifdef __cplusplus
}
#endif
#endif /* HRT_TESTING_H */
