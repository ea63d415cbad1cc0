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

/* The per-tile primary candidate lists of the sphere program's k_trace_split<true, false, false, false> (a listed tile's
 *   primary rays are answered and shaded when their frame block is made; same image, same queries).
 * mode: 0 the renderer's rule (on wherever that kernel draws with a bounce cap of at least 1), 1 off, 2 on (the same rule:
 *   other kernels never read lists). k: entries a list may hold, 0..8; a tile with more candidates is marked "walk" and
 *   its blocks walk their primary rays. RT_ERR_ARG outside those ranges. Stays set until changed; a new renderer
 *   starts with 0 and 8. */
int rt_testing_set_tile_lists(rt_renderer *r, uint32_t mode, uint32_t k);

/* Blocking read-back of the lists for the renderer's camera, spheres, size, row share and k (built now if the renderer
 *   does not hold them): 9 words per 8x8 tile, raster order over the renderer's rows: the count, or 0xFFFFFFFF for a
 *   tile marked "walk", then the BVH codes (positions in BVH order, rt_testing_sphere_bvh_leaves) ascending, then zeros.
 *   count: the words, always written. With cap 0 only the count is returned; a smaller cap otherwise is RT_ERR_ARG. */
int rt_testing_get_tile_lists(rt_renderer *r, uint32_t *words_out, size_t cap, size_t *count);

/* The frame blocks of the last draw (all its launches) whose primary rays k_trace_split answered and shaded when it made
 *   them; 0 for a draw that walked every primary ray (lists off, another kernel, every tile marked "walk"). Waits for
 *   the draw, as rt_get_stats. */
int rt_testing_get_tile_lists_resolved(rt_renderer *r, uint64_t *blocks);

/* The same lists on the host, no device: the rule is one inline function host and device both compile (f64, +, -, *, /
 *   and sqrt alone), so the device lists equal these byte for byte. camera80, spheres48, min_sphere_slots: as
 *   rt_set_camera, rt_set_spheres and rt_params; row0, row_step, row_block: the row share of rt_params (a whole image: 0,
 *   1, 1). count and cap as above. RT_ERR_ARG: a null pointer, a zero width, height or row_step, k above 8. */
int rt_host_tile_lists(const void *camera80, uint32_t width, uint32_t height, uint32_t row0, uint32_t row_step,
                       uint32_t row_block, const void *spheres48, uint32_t n, uint32_t min_sphere_slots, uint32_t k,
                       uint32_t *words_out, size_t cap, size_t *count);

/* The leaves of the sphere culling BVH the renderer would build over n_slots slots (centers_radii: cx, cy, cz, radius per
 *   slot, padding slots as zeros). Host only, no device.
 * leaves: one word per leaf in BVH order, first << 4 | count (first: the leaf's first position in BVH order).
 * slots: the slot of every BVH position, then the slots of the large list (scanned for every ray, not in the tree).
 * counts: {leaves, BVH positions, large-list entries, tree depth}; always written. With both capacities 0 only the
 *   counts are returned; a capacity that is too small otherwise is RT_ERR_ARG. */
int rt_testing_sphere_bvh_leaves(const float *centers_radii, uint32_t n_slots, uint32_t *leaves, uint32_t leaf_cap,
                                 int32_t *slots, uint32_t slot_cap, uint32_t counts[4]);

/* Blocking read-back of the triangle tree the renderer walks with tri_bvh = 1 or with device geometry, in the format
 *   and with the capacity rules of rt_host_lbvh_build_with (info[1] = info[2] = the leaf positions; info[5], [6] the
 *   PLOC iteration counts of device geometry built with RT_TREE_PLOC, else 0). A host SAH tree that
 *   was not built yet (rt_set_bvh, no tri_bvh = 1 query so far) is built first. RT_ERR_ARG in the sphere program. */
int rt_testing_get_tri_tree(rt_renderer *r, void *hnodes_out, size_t hnode_cap, uint32_t *order_out, size_t order_cap,
                            uint32_t info[8], float root[4]);

/* Blocking read-back of what cost-ordered dealing (rt_params.cost_order) has learnt: per tile (8x8 pixels, raster order
 *   over the renderer's rows) the sum of its pixels' cost counters from the last learning launch — a finished sample adds
 *   its bounces + 1 to its pixel — and the tile order built from the sums, a permutation of the tiles. count: the tiles
 *   the renderer holds an order for (0 before the first learning launch), always written. With cap 0 only the count is
 *   returned; a smaller cap otherwise is RT_ERR_ARG. */
int rt_testing_get_tile_order(rt_renderer *r, uint32_t *sum_out, uint32_t *order_out, size_t cap, size_t *count);

/* on != 0: rt_closest_points launches the counting instantiation of its kernel (k_closest_points<true>: the same walk
 *   and the same records, plus four sums per wave added to four words with one agent-scope atomic each); 0: the product
 *   kernel, which holds no counting code. Stays set until changed; a new renderer starts with 0. */
int rt_testing_set_closest_count(rt_renderer *r, uint32_t on);
/* Blocking: the four words of the last rt_closest_points call made with counting on (zeros before the first): {queries,
 *   point-triangle tests, queries that overflowed the walk's stack and finished with the loop over all triangles, queries
 *   that took that loop instead of the walk because the walk's error bound does not cover the point}. */
int rt_testing_get_closest_counts(rt_renderer *r, uint64_t out[4]);

/* on != 0: rt_winding_numbers launches the counting instantiation of its kernel (k_winding<true>: the same walk and the
 *   same bytes, plus five sums per wave added to five words with one agent-scope atomic each); 0: the product kernel,
 *   which holds no counting code. Stays set until changed; a new renderer starts with 0. */
int rt_testing_set_winding_count(rt_renderer *r, uint32_t on);
/* Blocking: the five words of the last rt_winding_numbers call made with counting on (zeros before the first): {queries,
 *   triangle terms (the flat definition's m included where a query took it), dipole terms, queries that overflowed the
 *   walk's stack, points the walk does not cover (non-finite ones included)}. */
int rt_testing_get_winding_counts(rt_renderer *r, uint64_t out[5]);
/* Blocking: the moments rt_winding_numbers reads (made first if the tree changed since), 64 B per node slot as
 *   rt_host_tree_moments writes them. *count = node slots (0 for a tree without nodes); moment_cap = 0 asks for the count
 *   alone, a smaller cap otherwise is RT_ERR_ARG. Programs and states as rt_winding_numbers. */
int rt_testing_get_tree_moments(rt_renderer *r, void *moments_out, size_t moment_cap, size_t *count);
/* Pure CPU: out[i] = csrc/rt_winding.hpp's written-out atan2 of (y[i], x[i]), the function host and device compile. */
int rt_testing_winding_atan2(const float *y, const float *x, uint32_t n, float *out);

/* on != 0: rt_cast_rays_multi launches the counting instantiation of its kernel (k_cast_rays_multi<., true>: the same walk
 *   and the same bytes, plus four sums per wave added to four words with one agent-scope atomic each); 0: the product
 *   kernel, which holds no counting code. Stays set until changed; a new renderer starts with 0. */
int rt_testing_set_multihit_count(rt_renderer *r, uint32_t on);
/* Blocking: the four words of the last rt_cast_rays_multi call made with counting on (zeros before the first): {queries,
 *   triangle tests (all m triangles for a query that ran the loop over all triangles), box tests, queries that overflowed
 *   the walk's stack}. */
int rt_testing_get_multihit_counts(rt_renderer *r, uint64_t out[4]);

/* on != 0: rt_overlap_volumes launches the counting instantiation of its kernel (k_overlap<., ., true>: the same walk and
 *   the same bytes, plus four sums per wave added to four words with one agent-scope atomic each); 0: the product
 *   kernel, which holds no counting code. Stays set until changed; a new renderer starts with 0. */
int rt_testing_set_overlap_count(rt_renderer *r, uint32_t on);
/* Blocking: the four words of the last rt_overlap_volumes call made with counting on (zeros before the first): {queries,
 *   triangle tests (all m triangles for a query that ran the loop over all triangles), box tests, queries that overflowed
 *   the walk's stack}. */
int rt_testing_get_overlap_counts(rt_renderer *r, uint64_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* HRT_TESTING_H */
