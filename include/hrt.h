/*
 * hrt.h — C-ABI of the MI355X-native path tracer (drop-in for hucancode/hello-raytracing's per-pixel ray
 * loop). Plain pointers, sizes and int status codes; no C++ or torch types cross this boundary.
 *
 * Two groups of entry points:
 *   rt_*  (renderer)  replace the wgpu Renderer + bind-group ABI + WGSL fs_main of the reference
 *                     (src/renderer.rs, src/shaders/shader_{sphere,tris}.wgsl). Backed by HIP kernels
 *                     for gfx950; they fail with RT_ERR_DEVICE when no MI355X is present — there is
 *                     no CPU fallback.
 *   rt_host_* (scene) host-side builders whose output bytes feed the renderer: Camera::new, Mesh::load_obj,
 *                     Tree::add_mesh/build, render_ppm, compare_ppm_images. Pure CPU.
 *
 * Every input buffer uses the reference's #[repr(C)] bytemuck POD layout byte for byte:
 *   Camera   80 B  {eye, direction, up, right: vec4<f32>; params: (focal, blur, fov, 0)} src/scene/camera.rs:6-12
 *   Material 32 B  {albedo: vec4<f32>; params: vec3<f32>; kind: u32}                      src/scene/material.rs:9-13
 *   Sphere   48 B  {center: vec3<f32>; radius: f32; material: Material}                   src/scene/sphere.rs:6-10
 *   Node     32 B  {bound_min: vec4<f32>; bound_max: vec4<f32>}                          src/scene/bvh/node.rs:6-9
 *   Triangle 64 B  {a, b, c: vec4<f32>; custom(normal): vec3<f32>; material: u32}       src/scene/bvh/triangle.rs:7-13
 * The callee copies every input (caller keeps ownership), as wgpu's queue.write_buffer does
 * (renderer.rs:350-353). One handle must not be used from two threads at once. A renderer stays on the
 * GPU that was current when it was created: every call that touches the device makes that GPU current for
 * its duration and restores the caller's current device before returning.
 */
#ifndef HRT_H
#define HRT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (the reference panics via unwrap/expect instead, e.g. renderer.rs:64,83,117) ---- */
#define RT_OK 0
#define RT_ERR_ARG (-1)      /* null pointer, zero size, bad mode, size mismatch                   */
#define RT_ERR_DEVICE (-2)   /* no gfx950 device / HIP runtime error                               */
#define RT_ERR_ALLOC (-3)    /* device or host allocation failed                                   */
#define RT_ERR_STATE (-4)    /* call out of protocol order (e.g. draw before camera)               */
#define RT_ERR_PARSE (-5)    /* OBJ parse error (tobj LoadError)                                   */
#define RT_ERR_COMPARE (-6)  /* compare_ppm_images failed (see rt_host_compare_ppm)                */

/* ---- scene modes: which WGSL program the renderer runs ---- */
#define RT_MODE_SPHERE 0 /* shader_sphere.wgsl: sphere list, BOUNCE_MAX 10, EPSILON 1e-6             */
#define RT_MODE_TRIS 1   /* shader_tris.wgsl: implicit-heap BVH of triangles, BOUNCE_MAX 5, EPS 1e-4 */
#define RT_MODE_MIXED 2  /* build-defined union (tris constants + sphere list), DESIGN.md §Mixed     */

/* Material kinds, src/scene/material.rs:4-6 */
#define RT_LAMBERTIAN 1u
#define RT_METAL 2u
#define RT_DIELECTRIC 3u

#define RT_MAX_OBJECT_IN_SCENE 100u /* scene_sphere.rs:15 — sphere buffer capacity = arrayLength */
#define RT_SAMPLE_FRAME 1000u        /* shader_*.wgsl SAMPLE_FRAME: EMA cap of the accumulation     */

typedef struct rt_renderer rt_renderer;

/* Runtime knobs that are compile-time constants in the WGSL (shader_sphere.wgsl:3-12). */
typedef struct rt_params {
    uint32_t bounces;          /* BOUNCE_MAX; default 10 (sphere) / 5 (tris, mixed)                     */
    uint32_t ema_cap;          /* SAMPLE_FRAME; default 1000                                          */
    uint32_t min_sphere_slots; /* arrayLength(&scene) floor; default 100 (zero-filled slots traced)    */
    uint32_t row0, row_step;   /* this renderer owns rows row0, row0+row_step, ... (multi-GPU tiles); with
                                  row_block > 1 the blocks of row_block rows starting there (below)    */
    uint32_t frames_per_launch;/* frames fused into one kernel launch by rt_draw_frames (default 32)   */
    uint32_t variant;          /* sphere-scan kernel: 0 auto (4 from 32 slots, 3 from 9, else 1), 1 simple,
                                  3 packed + deferred exact candidates, 4 conservative culling BVH;
                                  all bit-identical. 2 and 5-10 were removed.    */
    uint32_t schedule;         /* work schedule of rt_draw / rt_draw_frames: 0 auto (queue from 1.5M
                                  samples per draw, else tiles), 1 tiles (one lane per pixel for a
                                  launch's frames, in-register accumulation), 2 sample queue (persistent
                                  grid pulling 8x8-tile x job_frames jobs, colours folded in frame
                                  order); bit-identical                       */
    uint32_t queue_budget_mb;  /* sample-queue colour memory: 0 (default) auto = the sample buffer in
                                  floor(frames / 320) balanced launches of whole jobs (at least one), or as
                                  many frames per launch as 8 GiB holds if that is more, at most 32 GiB
                                  (C3: 352 + 352 + 320 frames, 8.8 GB; a rank of an 8-way C3: one launch);
                                  else a cap in MiB: balanced launches of as many frames as it holds. The
                                  fold ring (bounded memory, slower) when a launch would get fewer than
                                  min(frames, 320) frames                                 */
    uint32_t job_frames;       /* sample queue: frames per job (a job = one 8x8 tile), rounded down to a
                                  power of two (at most 1024); default 0 = per kernel: 32 with the
                                  suspendable walks, 16 for the linear sphere scans                      */
    uint32_t tri_bvh;          /* triangle program: 0 the reference's implicit-heap walk (default,
                                  parity), 1 opt-in binned-SAH tree with an ordered culling walk — the
                                  same closest hit except where the reference's 600-step cap or
                                  unpadded slab tests drop a triangle (non-parity).
                                  Not read after rt_set_triangles_device: a renderer with device geometry
                                  has no heap and walks its device-built tree with the kernels of 1,
                                  until rt_set_bvh gives it a heap again                             */
    uint32_t suspend_below;    /* sample queue: a wave suspends its walks (sphere culling BVH of the sphere
                                  program; reference heap walk of the triangle / mixed programs) once
                                  fewer than this many of its 64 lanes are still walking, so finished
                                  lanes shade and start their next query instead of idling (0 = no wave
                                  leaves a walk before all of its lanes finish); default 24 (sphere and
                                  mixed) / 32 (triangle); not used by tri_bvh = 1 or the linear sphere scans.
                                  Bit-identical either way                      */
    uint32_t row_block;        /* rows per block of the row partition (default 1; 0 reads as 1): the renderer
                                  owns rows row0 + k*row_step*row_block + j, j < row_block, in that order.
                                  Rank r of N with row_block 8 and row0 = 8r, row_step = N owns whole
                                  8-row tile rows dealt round-robin (bench.py)            */
    uint32_t fold;             /* sample queue colour fold: 0 auto (by queue_budget_mb, above; with the automatic
                                  budget, draws of two or more launches of the suspendable-walk kernels fold as 3),
                                  1 the sample buffer + k_accumulate after every launch, 2 the fold ring (bounded
                                  memory), 3 two sample buffers: each launch's waves fold the launch before it (1 in
                                  64 waves first folds tiles, then traces), k_accumulate the last launch only —
                                  twice the colour memory of 1 (C3 17.5 GB), C3 +1 %;
                                  k_trace's draws fold as 1; bit-identical                               */
    uint32_t heap_lds;         /* triangle / mixed programs: the top of the implicit heap in LDS, 0 auto = on,
                                  1 off (every node from L1/L2), 2 on: nodes 1..1023 as sign-ordered nodes
                                  (768-lane workgroups; nodes 1..255 with the deferred sphere scan; heaps of
                                  at most 2^24 nodes); bit-identical always                               */
    uint32_t steal;            /* sample queue with the sample buffer, suspendable-walk kernels: frame-block work
                                  stealing (a wave whose job queue is drained claims single frames of other
                                  waves' jobs, so no long job trails the launch): 0 auto = on for launches of
                                  fewer than 16 jobs per resident wave, 1 off, 2 on; bit-identical always  */
    uint32_t tail_split;       /* suspendable-walk kernels (k_trace_split, k_trace_split_tris) with the sample
                                  buffer and no stealing: the launch's last ~2 jobs per resident wave are dealt
                                  in parts, so the drain waits for a part of a job: 0 auto (quarters), 1 off,
                                  2 quarters, 3 eighths (job_frames a multiple of the part count);
                                  bit-identical                                                          */
    uint32_t count_tests;      /* 1: count the sphere program's culling-walk box and sphere tests
                                  (rt_stats.box_tests / sphere_tests); 0 (default): the sphere program's
                                  k_trace_split does not count them (reported 0; 1.3 % of C3's kernel
                                  time); the other kernels always count                                  */
    uint32_t cost_order;       /* sample queue with the sample buffer: deal a launch's most expensive tiles first
                                  (half of them, sorted by the queries their samples took in a learning launch;
                                  then the rest in raster order), so the slowest jobs do not trail
                                  the launch. The first launch after a change of scene, camera, size, rows,
                                  bounce cap, sphere slots or triangle walk learns (and deals in the last order
                                  learnt, or raster order).
                                  0 auto = on for a rank's share of a row partition (row_step > 1), which then
                                  does not steal once it has learnt, and for the suspendable-walk kernels (not
                                  the linear scans' full images), 1 off, 2 on, 3 on with every launch learning;
                                  bit-identical always                           */
    uint32_t packet;           /* sphere program, culling BVH with its nodes in LDS (k_trace_split): walk each frame
                                  block's 64 primary rays as one coherent packet when the block is made (one
                                  wave-uniform traversal of the union of their nodes) and hand the samples out with
                                  their first hit resolved: 0 auto = off, 1 off, 2 on; bit-identical images and
                                  query counts (box / sphere test counts then count the packet's tests). Off by
                                  default: C3 35.2 vs 38.3 Grays/s                 */
} rt_params;

#define RT_FOLD_AUTO 0u
#define RT_FOLD_BUFFER 1u
#define RT_FOLD_RING 2u
#define RT_FOLD_NEXT 3u

#define RT_SCHEDULE_AUTO 0u
#define RT_SCHEDULE_TILES 1u
#define RT_SCHEDULE_QUEUE 2u

typedef struct rt_stats {
    uint64_t queries;      /* closest-hit queries (rays) traced by the last draw call                  */
    uint64_t samples;      /* pixel-samples (pixels x frames) of the last draw call                    */
    double kernel_ms;      /* HIP-event time of the last draw call's kernels, on the renderer stream   */
    uint32_t launches;     /* kernel launches of the last draw call                                    */
    uint32_t local_rows;   /* rows owned by this renderer                                              */
    uint64_t box_tests;    /* padded-box tests of the sphere culling BVH (variant 4), last draw call    */
    uint64_t sphere_tests; /* ray-sphere tests (slots scanned, or BVH leaf + large-list tests)          */
    uint32_t variant;      /* sphere-scan variant the last draw call ran (1, 3, 4)                       */
    uint32_t schedule;     /* schedule the last draw call ran (RT_SCHEDULE_TILES / _QUEUE)             */
    uint64_t node_tests;   /* triangle program: implicit-heap node (slab) tests                         */
    uint64_t tri_tests;    /* triangle program: Moller-Trumbore tests                                   */
    double trace_ms;       /* HIP-event time of the ray-tracing kernels alone (k_render / k_trace)      */
    uint32_t trace_launches; /* launches of those kernels (the dominant kernel's launch count)          */
    uint32_t suspend_below; /* walks suspended below this many walking lanes in the last draw (k_trace_split*);
                              0 = every query ran to completion (k_trace, k_render)                    */
    char kernel[64];       /* the ray-tracing kernel the last draw ran, as rocprofv3 names it without
                              "void " and the argument list, e.g. "k_trace_split<true>"                 */
    uint64_t fold_bytes;   /* device memory the sample queue's colour fold used in the last draw: the sample
                              buffer (frames per launch x pixels x 12 B) or the fold ring (job slots x
                              job_frames x 64 px x 16 B plus control words); 0 for the tiles schedule    */
    uint32_t fold_ring;    /* 1: the last draw folded through the fold ring (bounded memory), 0: through the
                              sample buffer and k_accumulate, 2: through two sample buffers, each launch folded
                              inside the next (rt_params.fold 3; rt_params.queue_budget_mb decides)        */
    uint32_t launch_frames; /* sample queue: frames per trace launch of the last draw (the last launch may
                              have fewer; rt_params.queue_budget_mb)                                   */
    uint64_t device_bytes; /* device memory the renderer holds after the last draw call (image, scene,
                              colour fold, counters): the fold's share stays within queue_budget_mb      */
    uint32_t ordered_launches; /* trace launches of the last draw that dealt their tiles in cost order
                              (rt_params.cost_order)                                                    */
    uint32_t reserved;
} rt_stats;

/* Renderer::new(RenderOutput::Headless(w, h), ..) — renderer.rs:46-269. Zeroes the image (:249-257),
 * frame_count = 0. Selects the program (mode) like include_str!(shader) does (scene_sphere.rs:186).
 * A width or height of 1 (here or in rt_resize) draws what the reference draws: make_ray divides by W - 1 and H - 1, so
 * every primary ray and every pixel is NaN, every sample takes exactly one query, and the draw finishes. (With tri_bvh = 1
 * or a device tree such a ray hits the last triangle with t = NaN at every bounce — the rule for non-finite rays under
 * rt_cast_rays — so a sample takes rt_params.bounces queries; the pixel is NaN all the same.) */
int rt_create(uint32_t width, uint32_t height, int mode, rt_renderer **out);
int rt_destroy(rt_renderer *r);
int rt_get_params(const rt_renderer *r, rt_params *out);
/* Changing row0/row_step re-allocates and zeroes the image (like resize). */
int rt_set_params(rt_renderer *r, const rt_params *p);

/* Renderer::set_camera — renderer.rs:324-328 (group0 binding 4, 80 B). */
int rt_set_camera(rt_renderer *r, const void *camera80);
/* SceneSphere::write_scene_data -> Renderer::write_buffer(data, 0) — scene_sphere.rs:24-31,
 * renderer.rs:350-353 (group1 binding 0). n spheres of 48 B; slots past n are zero, like the wgpu buffer. */
int rt_set_spheres(rt_renderer *r, const void *spheres48, uint32_t n);
/* SceneTris::write_tree_data — scene_tris.rs:21-44 (group1 bindings 0..3): sizes = [n, m] (bvh_tree_size),
 * n Node (index 0 unused), m Triangle, k Material. n must be a power of two, as Tree::build makes it
 * (tree.rs:38, m.next_power_of_two()), and at most RT_MAX_TREE_NODES (the kernels read nodes and triangles
 * through buffer descriptors with 32-bit byte offsets: n x 32 B and m x 64 B stay below 4 GiB); RT_ERR_ARG
 * otherwise (rt_host_check_bvh_sizes applies the same rules without a device). */
int rt_set_bvh(rt_renderer *r, const uint32_t sizes[2], const void *nodes32, uint32_t n_nodes,
               const void *tris64, uint32_t n_tris, const void *mats32, uint32_t n_mats);
#define RT_MAX_TREE_NODES (1u << 26) /* 2^26 nodes (2 GiB), up to 2^26 - 1 triangles (4 GiB)            */

/* ---- device geometry (no reference counterpart: the reference builds its tree on CPU threads) ----
 * Triangles the caller keeps in device memory, for the triangle and mixed programs: n_tris Triangle records of 64 B, in
 * the layout rt_set_bvh takes, in device memory on the renderer's GPU, 16-byte aligned; n_mats Material records in HOST
 * memory, processed as rt_set_bvh processes them. The call makes the kernels' triangle records, builds an LBVH over the
 * triangles on the GPU, in the node format of the tri_bvh = 1 walk, and leaves the renderer in a device-geometry state:
 * it holds the triangles and that tree and no reference heap, and every draw and every query runs the kernels of
 * tri_bvh = 1 whatever rt_params.tri_bvh says (rt_set_params rebuilds nothing). rt_set_bvh leaves the state. The hit
 * contract is the one of tri_bvh = 1: the closest hit is the (t, triangle index) lexicographic minimum with the
 * reference's Moller-Trumbore arithmetic, and rt_hit.prim is the index into the caller's array.
 * The builder (csrc/rt_lbvh.hpp has every rule, DESIGN.md §7d the reasons): e1 = b - a, e2 = c - a in f32; f64 boxes over
 * a, a + e1, a + e2; a triangle with a non-finite vertex stays out of the tree; 30-bit Morton keys of the f64 centroids
 * in the root box; a stable sort; Karras' topology with index tie-break; children of at most 4 triangles become leaves;
 * boxes fitted bottom-up in f64 and packed outward to fp16. The tree is a pure function of the triangle array:
 * rt_host_lbvh_build gives the same bytes on the host.
 * The call copies what it needs (the caller may overwrite tris64_dev after it returns) and is synchronous on the
 * renderer's stream, like rt_set_bvh: it ends by reading a small status block back. The caller must have finished
 * writing the triangles (the Python wrapper synchronises torch's current stream first).
 * RT_ERR_ARG: the sphere program; a null tris64_dev with n_tris > 0; a pointer that is not 16-byte aligned;
 * n_tris >= 2^26 or n_mats >= 2^28; a null mats32 with n_mats > 0; any triangle whose material >= n_mats (counted on the
 * device). On any failure the renderer keeps the geometry it had: the build works in staging buffers that are swapped in
 * on success. Those and the build's scratch count in rt_stats.device_bytes; rt_release_scratch frees them, not the tree.
 * The image, the frame count and rt_get_stats are not touched; the learnt cost order is dropped, as by rt_set_bvh. */
int rt_set_triangles_device(rt_renderer *r, const void *tris64_dev, uint32_t n_tris, const void *mats32,
                            uint32_t n_mats);
/* The same call with the topology builder named. RT_TREE_LBVH is rt_set_triangles_device exactly (which is this call with
 * it). RT_TREE_PLOC keeps everything up to the sort and everything after the topology (the fit, the packing, the root
 * sphere, the refit, the cost read-out, the walk) and replaces Karras' construction by parallel locally-ordered clustering
 * (Meister and Bittner 2018) over the sorted order; csrc/rt_lbvh.hpp states it as a pure function, DESIGN.md §7d has the
 * reasons and the measurements. In words: one cluster per sorted position p (the triangle's f64 box, the leaf word
 * 0x80000000 | p << 4 | 1: every leaf holds ONE triangle); per iteration every cluster i finds, among the up to 8 clusters
 * on each side, the j with the smallest (half-area of the union box, i XOR j), and i, j merge when each is the other's
 * choice; the s-th of an iteration's k pairs, in list order, becomes node next - k + s (next: the ids not given out, m' - 1
 * at first), so node 0 is the root, all m' - 1 slots are referenced and a child's index is above its parent's; the merged
 * cluster stays in the lower partner's place. An iteration t with t + ceil(log2(clusters)) >= 64 takes every distance as 0
 * ("flat": clusters 2 s and 2 s + 1 merge), which bounds the build at 64 iterations and the tree at 64 levels. m' <= 4
 * finite triangles give builder 0's tree (one leaf word, no nodes). The tree is slower to build (it reads a cluster count
 * back per iteration until 1024 clusters are left) and cheaper to walk; its depth may exceed the walk's stack of 24, which
 * the walk's overflow path answers correctly and slowly: rt_get_tri_tree_info reports the depth.
 * RT_ERR_ARG also for an unknown builder; everything else (arguments, staging, failure keeps the geometry, synchronous,
 * rt_stats.device_bytes, rt_release_scratch) is rt_set_triangles_device's. */
#define RT_TREE_LBVH 0u
#define RT_TREE_PLOC 1u
#define RT_TREE_HOST_SAH 0xFFFFFFFFu /* reported by rt_get_tri_tree_info for the host tree of tri_bvh = 1; not a builder argument */
int rt_set_triangles_device_with(rt_renderer *r, const void *tris64_dev, uint32_t n_tris, const void *mats32,
                                 uint32_t n_mats, uint32_t builder);
/* The same builder on the host, for n_tris Triangle records in host memory: pure CPU, no device, usable without a GPU,
 * and what the tests compare the device tree with. hnodes_out: 32 B per node slot (per child six fp16 box bounds relative
 * to the root centre, [min | max << 16] per axis, then the child word: a node index, or
 * 0x80000000 | first << 4 | count for a leaf of `count` entries of order_out from `first`); slots no child word names
 * are zero. order_out: the finite triangles' indices in key order. Capacities in node slots and in words.
 * info: {node slots, leaf positions, finite triangles, root word, depth, 0, 0, 0}; root: {centre xyz, radius}; both are
 * always written. With both capacities 0 only they are returned; a capacity that is too small otherwise is RT_ERR_ARG. */
int rt_host_lbvh_build(const void *tris64, uint32_t n_tris, void *hnodes_out, size_t hnode_cap, uint32_t *order_out,
                       size_t order_cap, uint32_t info[8], float root[4]);
/* The same with the builder named: RT_TREE_LBVH is rt_host_lbvh_build's bytes; RT_TREE_PLOC is the host mirror of
 * rt_set_triangles_device_with's tree, with info[5] = iterations run and info[6] = how many of them were flat (both 0
 * for builder 0 and for a tree without nodes). RT_ERR_ARG for an unknown builder. */
int rt_host_lbvh_build_with(const void *tris64, uint32_t n_tris, uint32_t builder, void *hnodes_out, size_t hnode_cap,
                            uint32_t *order_out, size_t order_cap, uint32_t info[8], float root[4]);
/* Refit: the moved positions of a mesh that keeps its connectivity, on the tree of the last successful
 * rt_set_triangles_device. tris64_dev: the same records as there (64 B each, device memory on the renderer's GPU, 16-byte
 * aligned); n_tris must equal that build's count. Kept: the build's topology, that is the sorted order, the parent links
 * and every child word, so a leaf holds the triangle indices it held. Recomputed with the build's own rules, from the array
 * given now: the kernels' triangle records (custom normal and material index included), the per-triangle f64 boxes, the
 * root box, centre and radius, every referenced node's two packed child boxes (relative to the NEW root centre), the
 * depth (which comes out the same). The materials table is not touched: a material index >= the count given to the build
 * is an error. A tree without nodes (<= 4 finite triangles) changes only its triangle records and root sphere.
 * The refitted tree is a pure function of two arrays: the topology of the array of the last successful build, the boxes of
 * the array given now. build(A), refit(B), refit(C) leaves the bytes of rt_host_lbvh_refit(A, C); a refit with the
 * unmoved array leaves the build's bytes. The hit contract does not depend on the tree's shape: every query and draw
 * returns bit for bit what a fresh rt_set_triangles_device on the new array returns; only the speed may differ, and it
 * gets worse as the mesh leaves the pose the tree was built for (rt_get_tri_tree_cost says how much; the caller decides
 * when to build again). One memset, two kernels and the status read-back: no keys, no sort, no topology.
 * RT_ERR_ARG: the sphere program; a null tris64_dev with n_tris > 0; a pointer that is not 16-byte aligned; n_tris other
 * than the built count; a material index out of range; a triangle that changed finiteness either way (the set of
 * triangles with a non-finite a, e1 or e2 must be the one the topology was built over; counted on the device, the
 * message has the count). RT_ERR_STATE: no device geometry (never set, or rt_set_bvh left the state). On any failure the
 * renderer keeps the geometry it had: the refit writes the staging set and swaps it in on success. The parent links are
 * part of the tree (counted in rt_stats.device_bytes, kept by rt_release_scratch, untouched by a build that fails): a
 * refit after rt_release_scratch allocates staging and scratch again, a refit after a failed build uses the live tree.
 * Synchronous on the renderer's stream like the build; drops the learnt cost order; image, frame count and rt_get_stats
 * are not touched. The refit reads the live topology whichever builder made it: its host mirror is
 * rt_host_lbvh_refit_with with the builder of the last successful build. */
int rt_refit_triangles_device(rt_renderer *r, const void *tris64_dev, uint32_t n_tris);
/* The refit on the host: the topology rt_host_lbvh_build gives tris64_topology, the boxes of tris64 (n_tris records each,
 * host memory). Outputs, capacities and the two-call protocol are rt_host_lbvh_build's. RT_ERR_ARG also when a triangle
 * is finite in one array and not in the other. rt_host_lbvh_refit(A, A) is rt_host_lbvh_build(A). */
int rt_host_lbvh_refit(const void *tris64_topology, const void *tris64, uint32_t n_tris, void *hnodes_out,
                       size_t hnode_cap, uint32_t *order_out, size_t order_cap, uint32_t info[8], float root[4]);
/* The same on the topology rt_host_lbvh_build_with(tris64_topology, builder) gives; info as there. */
int rt_host_lbvh_refit_with(const void *tris64_topology, const void *tris64, uint32_t n_tris, uint32_t builder,
                            void *hnodes_out, size_t hnode_cap, uint32_t *order_out, size_t order_cap, uint32_t info[8],
                            float root[4]);
/* Tree cost: a deterministic read-out of any tree in the node format above (the host SAH tree of tri_bvh = 1 included),
 * in integers, so that no summation order can matter; a pure function of the bytes. A referenced node is a slot whose left
 * child word is not 0. Per child of one: the six halves decoded to f64; per axis e = hi - lo, 0 if !(e > 0), 131008 if
 * e > 131008 (inf halves); A = e_x e_y + e_y e_z + e_z e_x, products and sums rounded in that order, no FMA. R is the same
 * expression over the union of the two child boxes of the node root_word names. q = R > 0 ? min((uint64_t)(A / R *
 * 65536.0), 2^32) : 0 (IEEE division). cost[0] = sum of q over children that are nodes; cost[1] = sum of q x count over
 * leaf children; cost[2] = referenced nodes; cost[3] = leaf entries (sum of count). A root word that is a leaf gives four
 * zeros. The usual SAH figure is (cost[0] + cost[1]) / 65536. RT_ERR_ARG: a root word that names a node >= node_slots. */
int rt_host_lbvh_cost(const void *hnodes, size_t node_slots, uint32_t root_word, uint64_t cost[4]);
/* The same read-out, by a small kernel, of the tree the renderer walks with tri_bvh = 1 or with device geometry (a host
 * SAH tree not built yet is built first). Blocking. RT_ERR_ARG in the sphere program. Touches nothing a draw reads. */
int rt_get_tri_tree_cost(rt_renderer *r, uint64_t cost[4]);
/* The triangle tree the renderer walks, in numbers: {builder, node slots, finite triangles, root word, depth, iterations,
 * flat iterations, 0}. builder: RT_TREE_LBVH or RT_TREE_PLOC with device geometry, RT_TREE_HOST_SAH for the host tree of
 * tri_bvh = 1 (built first if it is not yet); the two iteration counts are 0 unless PLOC built nodes. A depth above 24 means
 * that rays can leave the walk's stack for its slow overflow path. RT_ERR_ARG in the sphere program; RT_ERR_STATE when
 * there is no triangle tree (no device geometry and tri_bvh = 0). Touches nothing a draw reads. */
int rt_get_tri_tree_info(rt_renderer *r, uint32_t info[8]);

/* Renderer::set_time / set_frame_count — renderer.rs:315-323. */
int rt_set_time(rt_renderer *r, uint32_t time);
int rt_set_frame_count(rt_renderer *r, uint32_t frame_count);
int rt_get_frame_count(const rt_renderer *r, uint32_t *out);

/* Renderer::draw — renderer.rs:355-410: one frame (one sample per pixel) at the current time,
 * frame_count += 1. Asynchronous on the renderer's HIP stream. */
int rt_draw(rt_renderer *r);
/* `count` frames with time_f = time0 + f*dtime, frame_count advancing by one per frame: bit-identical
 * to count x {rt_set_time(time_f); rt_draw()}. The tiles schedule accumulates in registers in-kernel; the
 * sample queue stores each sample's colour (sample buffer or fold ring) and folds them in frame order with
 * the same expression (k_accumulate after the launch, or inside it), see rt_params.fold. */
int rt_draw_frames(rt_renderer *r, uint32_t count, uint32_t time0, uint32_t dtime);

/* render_ppm's copy_image_buffer — render_ppm.rs:7-36: blocking readback of the f32 RGB image,
 * row-major, (local_rows x width x 3) floats. */
int rt_read_image(rt_renderer *r, float *out, size_t n_floats);
/* Restore an accumulation state (checkpoint/resume: image + rt_set_frame_count). */
int rt_write_image(rt_renderer *r, const float *in, size_t n_floats);
/* Device-to-device copy of the image into caller memory on the caller's device (multi-GPU gather). */
int rt_copy_image_to_device(rt_renderer *r, void *dst_device, size_t n_floats);
/* Renderer::reset_frame_count / resize — renderer.rs:336-348, :271-313 (both zero the image). */
int rt_reset_frame_count(rt_renderer *r);
int rt_resize(rt_renderer *r, uint32_t width, uint32_t height);
int rt_synchronize(rt_renderer *r);
int rt_get_stats(const rt_renderer *r, rt_stats *out);
/* Frees the sample queue's colour-fold memory (the sample buffer or the fold ring, rt_stats.fold_bytes)
 * after the pending draws; the next queue draw allocates it again. For a renderer kept alive between
 * renders beside other work: one C3 render holds 8.8 GB under the default budget (352 frames x 24.9 MB;
 * rt_stats.fold_bytes has the figure of the last draw) (no reference counterpart: wgpu frees nothing
 * either, but the reference has no per-sample buffer). */
int rt_release_scratch(rt_renderer *r);

/* ---- ray queries (no reference counterpart: the reference traces only the rays fs_main makes for itself) ----
 * The closest-hit query of the render path — the sphere culling BVH or linear scans, the reference heap walk with its
 * 600-step cap, the opt-in SAH tree — for rays the caller keeps in device memory, and the primary rays a frame samples.
 * Neither call reads or changes the image, the frame count, rt_get_stats, the raw counters or the learnt cost order. */
#define RT_T_MISS 3.40282e+38f      /* the WGSL FLT_MAX: t of a ray that hit nothing */
#define RT_HIT_FRONT    1u          /* Hit.front as the running program computes it   */
#define RT_HIT_TRIANGLE 2u          /* prim indexes the triangle buffer, else a sphere slot */
typedef struct rt_hit {             /* 32 B */
    float t; int32_t prim;          /* miss: RT_T_MISS, -1, everything below 0 */
    float n[3];                     /* Hit.n of the render path (sphere: faced against the ray; triangle: as stored) */
    uint32_t flags, material, reserved; /* material: sphere slot, or Triangle.material */
} rt_hit;
/* n rays -> n rt_hit records. origins_dev / dirs_dev: n x 3 f32 each, packed (12-byte stride, 4-byte aligned);
 * hits_dev: n x 32 B, 16-byte aligned. All three are device memory on the renderer's GPU. Asynchronous on the renderer's
 * stream: rt_synchronize waits for it, and the caller orders its own streams against it (the buffers must be ready
 * before the call, and are not to be read before rt_synchronize).
 * The hit is exactly what one bounce of trace() would see for that ray in the renderer's program:
 *   - sphere program: d is not normalised, so t is in units of |d|; the near root only, t > 0;
 *   - triangle and mixed programs: triangles accept t >= 1e-4, and a triangle replaces a sphere only with a smaller t;
 *   - the reference heap walk keeps its 600-step cap (it may miss what the cap cuts off) unless tri_bvh = 1;
 *   - zero-filled padding slots (rt_params.min_sphere_slots) count as spheres of radius 0 at the origin;
 *   - a ray with a non-finite component is answered as trace() answers it. The sphere programs' tests refuse a NaN t. The
 *     reference heap walk's slab test drops a NaN axis (fmin / fmax) and its triangle test, `t < EPSILON || t >= hit.t`
 *     rejects, accepts a NaN t, so such a ray can hit with t = NaN, prim the last triangle the walk accepted; a NaN t held
 *     is replaced by the next t that is not below 1e-4, larger or not. With tri_bvh = 1 and on a device tree the hit of a
 *     finite ray is the (t, triangle index) minimum over t >= 1e-4; a ray with a NaN or infinite component is answered
 *     by the reference's rule over every triangle in index order, as if the heap walk reached every leaf: no box is tested
 *     for it. That costs the triangles after the last one whose t is NaN (none, for a NaN in d) and, for a ray no triangle
 *     gives a NaN t, every triangle twice.
 * rt_params.variant (0 = auto by slot count), tri_bvh and min_sphere_slots apply as in a tiles draw; the schedule, fold,
 * steal and cost-order knobs do not. n = 0 returns RT_OK and launches nothing; n > 0 with a null pointer is RT_ERR_ARG. A
 * scene state in which a draw fails gives the same status here; no camera is needed. */
int rt_cast_rays(rt_renderer *r, const void *origins_dev, const void *dirs_dev, uint32_t n, void *hits_dev);
/* The occlusion query: is anything in the way before distance tmax? n rays -> n bytes, 1 = occluded, 0 = not.
 * origins_dev / dirs_dev as rt_cast_rays (n x 3 f32, packed, 4-byte aligned); tmax_dev: n f32 (4-byte aligned) or NULL =
 * RT_T_MISS for every ray ("any hit at all"); occluded_dev: n bytes, no alignment. Device memory on the renderer's GPU,
 * asynchronous on the renderer's stream, as rt_cast_rays.
 * The whole contract: for the same renderer state and the same ray, byte i is 1 exactly when rt_cast_rays would return a
 * hit (prim >= 0) with t < tmax[i], as an f32 comparison. So everything rt_cast_rays documents carries over — the sphere
 * program's unnormalised d (tmax in units of |d|), triangles from t >= 1e-4, the reference walk's 600-step cap (a
 * triangle the capped walk never reaches does not occlude), zero padding slots counted as spheres, rt_params.variant /
 * tri_bvh / min_sphere_slots — and a hit at exactly t == tmax does not occlude. A NaN tmax, or any tmax <= 0 including
 * -0, gives 0; a tmax above RT_T_MISS (+inf, FLT_MAX) behaves as RT_T_MISS. Only the values 0 and 1 are ever written,
 * and exactly n bytes are written. A hit with t = NaN (rt_cast_rays, non-finite rays) is not below any tmax and does not
 * occlude; the walk refuses every NaN t and goes on. One case is therefore answered for the closest finite t instead of
 * rt_cast_rays' t: a ray for which some triangle tests give a NaN t and others a finite one, where the reference's rule
 * lets the NaN displace a smaller t it held.
 * A segment query from a to b is o = a, d = b - a, tmax = 1. In the triangle and mixed programs the triangle test's
 * absolute |det| >= 1e-4 makes the result depend on |d| (a short d can fall under it), as it does for rt_cast_rays.
 * The walks start at tmax instead of RT_T_MISS and stop at the first occluder, so a short ray skips most of the scene;
 * no hit record is built. n = 0 returns RT_OK and launches nothing; n > 0 with a null origins, dirs or occluded pointer,
 * or a misaligned f32 buffer, is RT_ERR_ARG. A scene state in which a draw fails gives the same status here; no camera
 * is needed. Like the calls beside it, it touches no image, frame count, stats, raw counters or learnt cost order. */
int rt_occluded(rt_renderer *r, const void *origins_dev, const void *dirs_dev, const void *tmax_dev, uint32_t n,
                void *occluded_dev);
/* The primary rays of the frame drawn at `time` (rt_set_time): for local row k and column x, ray k * width + x is the one
 * fs_main traces for that pixel — antialiasing jitter, lens offset and, in the triangle and mixed programs, the
 * normalised direction included — as 3 f32 origin and 3 f32 direction, packed like rt_cast_rays' inputs (device memory,
 * asynchronous on the renderer's stream). Needs a camera (RT_ERR_STATE otherwise, as drawing does); n_rays must equal
 * local_rows x width (RT_ERR_ARG otherwise). rt_cast_rays on them gives the first hit behind each pixel sample. */
int rt_primary_rays(rt_renderer *r, uint32_t time, void *origins_dev, void *dirs_dev, size_t n_rays);
/* The radiance query: n rays -> n radiances, the colour fs_main would mix into a pixel whose primary ray this is
 * (0.0 + trace(ray)): the whole multi-bounce path of the renderer's program for rays the caller makes.
 * origins_dev / dirs_dev as rt_cast_rays (n x 3 f32, packed, 4-byte aligned). rng_dev: n u32 (4-byte aligned), entry i
 * the RNG state ray i's path starts from — the `s` that scatter advances — or NULL = the state s_i = (i + 1) * seed in
 * u32 arithmetic (by analogy with the reference's (x * H + y) * time); seed is ignored when rng_dev is given, and rng_dev
 * is only read. radiance_dev: n x 3 f32, packed, 4-byte aligned; exactly 12 n bytes are written. queries_dev: n u32
 * (4-byte aligned) or NULL; it receives the number of closest-hit queries ray i's path took, 0 .. rt_params.bounces, and
 * exactly 4 n bytes are written when it is given. Device memory on the renderer's GPU, asynchronous on the renderer's
 * stream, as rt_cast_rays.
 * The path is exactly trace() of the renderer's program: each bounce is the query rt_cast_rays documents, then scatter,
 * then attenuation by albedo * 0.7, up to rt_params.bounces times; the sky term is taken from the GIVEN ray's d.y. In the
 * sphere program d is not normalised, so the caller's |d| enters the sky blend exactly as it would in trace().
 * Everything rt_cast_rays documents carries over — the sphere program's unnormalised d, triangles from t >= 1e-4 and the
 * |det| >= 1e-4 threshold, the reference walk's 600-step cap unless tri_bvh = 1, zero padding slots counted as spheres —
 * and rt_params.variant, tri_bvh, min_sphere_slots and bounces apply as in a tiles draw. bounces = 0 gives the sky colour
 * and 0 queries. So with the rays of rt_primary_rays and the states of rt_primary_rng for one `time`, the result is bit
 * for bit the image a one-frame draw at that time leaves from frame count 0, and the queries sum to its ray count.
 * n = 0 returns RT_OK and launches nothing; n > 0 with a null origins, dirs or radiance pointer, or a misaligned buffer,
 * is RT_ERR_ARG. A scene state in which a draw fails gives the same status here; no camera is needed. Like the calls
 * beside it, it touches no image, frame count, stats, raw counters or learnt cost order. */
int rt_trace_rays(rt_renderer *r, const void *origins_dev, const void *dirs_dev, const void *rng_dev, uint32_t seed,
                  uint32_t n, void *radiance_dev, void *queries_dev);
typedef struct rt_bounce {           /* every pointer: device memory on the renderer's GPU */
    void *origins_dev, *dirs_dev;    /* paths x 3 f32, packed (4-byte aligned): read; overwritten for a path that hit */
    void *rng_dev;                   /* paths u32: read; overwritten for a path that hit */
    void *throughput_dev;            /* paths x 3 f32 or NULL: multiplied by albedo * 0.7 for a path that hit */
    void *queries_dev;               /* paths u32 or NULL: += 1 for every path processed */
    void *hits_dev;                  /* paths x 32 B rt_hit (16-byte aligned) or NULL: this step's hit record */
    const void *index_in_dev;        /* n u32 path indices, or NULL = path i is entry i */
    const void *count_in_dev;        /* one u32, or NULL: only the first min(n, *count_in) entries are processed */
    void *index_out_dev;             /* room for n u32, or NULL: the indices of the paths that hit */
    void *count_out_dev;             /* one u32, or NULL (required with index_out): how many paths hit */
    uint32_t paths;                  /* entries in the state arrays; an index >= paths is skipped */
    uint32_t reserved;               /* 0 */
} rt_bounce;
/* The path step: ONE iteration of trace()'s loop for paths whose state (ray, RNG state, throughput) the caller keeps in
 * device memory between steps, with the paths that hit compacted into an index list for the next step — the wavefront
 * counterpart of rt_trace_rays, for a caller's own integrator (shadow rays by rt_occluded between steps, per-bounce
 * outputs, regrouping). Iterating it rt_params.bounces times from the rays of rt_primary_rays and the states of
 * rt_primary_rng, with throughput started at 1, leaves throughput * sky equal to rt_trace_rays' radiance bit for bit and
 * queries equal to its queries.
 * Entry i of the n entries is path j = index_in ? index_in[i] : i. Only the first min(n, *count_in) entries are processed
 * when count_in is given; an entry with j >= paths is skipped: nothing is read or written for it and it is not forwarded.
 * For each processed path j:
 *   - the query is the one rt_cast_rays documents, on (origins[j], dirs[j]): the sphere program's unnormalised d,
 *     triangles from t >= 1e-4 and the |det| >= 1e-4 threshold, the reference walk's 600-step cap unless tri_bvh = 1, zero
 *     padding slots counted as spheres, rt_params.variant / tri_bvh / min_sphere_slots; rt_params.bounces is not read (the
 *     caller decides how many steps to take);
 *   - on a hit, scatter advances rng[j] and replaces origins[j] and dirs[j], throughput[j] is multiplied component by
 *     component by (albedo.r * 0.7, albedo.g * 0.7, albedo.b * 0.7) (throughput on the left, as trace() attenuates), and
 *     j is appended to index_out and counted in *count_out;
 *   - on a miss, origins[j], dirs[j], rng[j] and throughput[j] are left untouched, bit for bit, and j is not forwarded;
 *   - either way queries[j] += 1, and hits[j] is the record rt_cast_rays would write for the ray BEFORE the scatter; both
 *     only when the buffer is given.
 * Compaction: *count_out is set to 0 on the renderer's stream before the kernel; index_out[0 .. *count_out - 1] receives
 * exactly the forwarded indices, each once, and nothing past them is written. Order: entries of one 64-lane wave (entries
 * 64 k .. 64 k + 63) keep their relative order; the order between waves is unspecified — compare as sets. count_out
 * without index_out only counts.
 * Aliasing: index_out must not overlap index_in and count_out must not be count_in: the caller ping-pongs between two
 * (index, count) pairs (count_out == count_in is refused; an overlap of the index lists is not checked). Duplicate indices in index_in are the caller's error: the result is undefined and
 * nothing checks for them.
 * count_in exists so that a loop of steps needs no host read-back: launch every step with the first step's n and hand
 * step k's count_out to step k + 1 as count_in.
 * Asynchronous on the renderer's stream, as rt_cast_rays. n = 0 returns RT_OK and launches nothing. RT_ERR_ARG: n > 0 with
 * a null io, origins, dirs or rng; index_out without count_out; index_in == NULL with n > paths; a misaligned buffer;
 * reserved != 0; count_out == count_in. A scene state in which a draw fails gives the same status here; no camera is
 * needed. Like the calls beside it, it touches no image, frame count, stats, raw counters or learnt cost order. */
int rt_bounce_rays(rt_renderer *r, const rt_bounce *io, uint32_t n);
#define RT_REGROUP_CELL_OCTANT 1u   /* 24-bit key from the path's ray and a caller's box (below) */
#define RT_REGROUP_KEYS        2u   /* 32-bit keys the caller supplies per path                  */
#define RT_REGROUP_MAX_ENTRIES (1u << 28)
#define RT_REGROUP_TILE        1024u /* entries per workgroup of the sort's count and scatter kernels */
typedef struct rt_regroup {          /* every pointer: device memory on the renderer's GPU */
    const void *origins_dev, *dirs_dev; /* paths x 3 f32, packed: read (mode 1); unused and may be NULL in mode 2 */
    const void *keys_dev;            /* paths u32, indexed by PATH: read (mode 2); unused and may be NULL in mode 1 */
    const void *index_in_dev;        /* n u32 path indices, or NULL = entry i is path i */
    const void *count_in_dev;        /* one u32 or NULL: only the first min(n, *count_in) entries are sorted */
    void *index_out_dev;             /* room for n u32: the same indices, in key order */
    void *keys_out_dev;              /* room for n u32 or NULL: the key of each output entry */
    uint32_t paths, mode;
    float box_lo[3], box_hi[3];      /* mode 1: the box the origins are quantised in */
    uint32_t reserved;               /* 0 */
    uint32_t pad;                    /* not read: makes sizeof 96, a multiple of the pointers' 8 bytes */
} rt_regroup;
/* Regrouping: sorts a path index list by a coherence key, on the device, so that the lanes of a wave of the next
 * rt_bounce_rays step walk neighbouring parts of the scene (or share whatever the caller's keys say they share). The live
 * count stays on the device and the result goes straight into the next step as index_in: no read-back, like count_in.
 * Entries: live = min(n, *count_in), or n without count_in. Entry i < live is path j = index_in ? index_in[i] : i.
 * Output: index_out[0 .. live - 1] is a permutation of those j in ascending key order; entries with equal keys keep their
 * input order (the sort is stable), so given its inputs the result is fully determined, bit for bit. keys_out[k], when
 * given, is the key of index_out[k]. Nothing is written at or past position live of either output, and no other buffer of
 * the caller's is written. There is no count_out: the count does not change, and the caller hands the same count buffer
 * to the next step.
 * Keys: an entry with j >= paths is kept, with the largest key of the mode (0x00FFFFFF in mode 1, 0xFFFFFFFF in mode 2), so
 * it sorts into the last group; nothing is read through such an index (rt_bounce_rays skips it later anyway). Duplicate
 * indices are not an error here: each entry is sorted on its own.
 *   RT_REGROUP_CELL_OCTANT (mode 1): 24 bits from (origins[j], dirs[j]) and the box, computed in f32 with no FMA, the same
 *     inline function on host and device. The host computes inv_k = 128.0f / (box_hi[k] - box_lo[k]) per axis (the IEEE
 *     division); per axis f = (o_k - box_lo[k]) * inv_k, two rounded operations, and
 *     q_k = !(f > 0) ? 0 : (f >= 128 ? 127 : (uint32_t)f), so NaN and -inf give 0 and +inf gives 127. Bit i of q_x, q_y, q_z
 *     goes to key bit 3 + 3i, 4 + 3i, 5 + 3i (a Morton code of the cell in a 128^3 grid over the box); key bits 0, 1, 2
 *     are the raw sign bits of d.x, d.y, d.z, read from the bit pattern (-0 and a negative NaN count as negative). The rays
 *     of one cell that point into the same octant end up next to each other. A bad box is RT_ERR_ARG: every
 *     box_hi[k] - box_lo[k] must be finite and >= 2^-60, and every inv_k finite. rt_host_regroup_keys gives the same keys
 *     on the host.
 *   RT_REGROUP_KEYS (mode 2): keys[j], all 32 bits (the material or primitive of rt_bounce's hits, a caller's own cell).
 * Aliasing: index_out == index_in, the same pointer, is allowed: regrouping in place between two steps (every read of
 * index_in happens before the first write of index_out). Any other overlap of the two is undefined. keys_out must not
 * overlap any input.
 * Scratch: the sort (a stable least-significant-digit radix sort over 8-bit digits, 3 passes in mode 1 and 4 in mode 2)
 * works in memory the renderer owns, grown on demand and kept for the next call: 4 u32 per entry of the largest n so far,
 * plus 256 u32 of digit counts per RT_REGROUP_TILE entries of it (rounded up), plus 1040 u32. rt_release_scratch and
 * rt_destroy free it.
 * Asynchronous on the renderer's stream, as rt_cast_rays; every kernel is launched for the caller's n and reads the count
 * on the device. n = 0 returns RT_OK and launches nothing. RT_ERR_ARG: a null io or index_out; a null origins or dirs in
 * mode 1; a null keys in mode 2; an unknown mode; reserved != 0; a misaligned buffer (4 bytes); index_in == NULL with
 * n > paths; n > RT_REGROUP_MAX_ENTRIES; a bad box in mode 1. It needs no scene and no camera and works in any scene
 * state. Like the calls beside it, it touches no image, frame count, stats, raw counters or learnt cost order. */
int rt_regroup_paths(rt_renderer *r, const rt_regroup *io, uint32_t n);
/* The key of mode 1 on the host, for n rays: pure CPU, no device. origins / dirs: n x 3 f32, packed; keys_out: n u32.
 * RT_ERR_ARG for a null pointer with n > 0 or a bad box (as rt_regroup_paths). */
int rt_host_regroup_keys(const float *origins, const float *dirs, uint32_t n, const float box_lo[3],
                         const float box_hi[3], uint32_t *keys_out);
/* The RNG state fs_main holds after make_ray for each pixel of the frame drawn at `time` (the companion of
 * rt_primary_rays: same pixel order, same row partition): n_rays u32, 4-byte aligned device memory, asynchronous on the
 * renderer's stream. Needs a camera (RT_ERR_STATE otherwise); n_rays must equal local_rows x width (RT_ERR_ARG
 * otherwise). */
int rt_primary_rng(rt_renderer *r, uint32_t time, void *rng_dev, size_t n_rays);
/* The renderer's HIP stream (a hipStream_t, created non-blocking; owned by the renderer, valid until rt_destroy): for a
 * caller that orders its own streams against the asynchronous calls above with events instead of rt_synchronize, or
 * times them (scripts/bench_cast.py). */
int rt_get_stream(const rt_renderer *r, void **hip_stream);

/* ---- point queries (no reference counterpart) ----
 * The nearest point of the triangle set for each of the caller's points, on the triangle tree the ray queries walk: how
 * far is this point from the surface, and where on it (contact and penetration tests, snapping and projection, chamfer
 * and point-to-surface losses, attaching particles to a skinned mesh). Unsigned: there is no inside or outside here. */
typedef struct rt_closest {         /* 32 B */
    float d2; int32_t prim;         /* squared distance, triangle index; miss: RT_T_MISS, -1, everything below 0 */
    float p[3];                     /* the closest point: a + (v e1 + w e2) */
    float v, w;                     /* weights of b and c; a's is 1 - v - w */
    uint32_t reserved;              /* 0 */
} rt_closest;
/* n points -> n rt_closest records. points_dev: n x 3 f32, packed (12-byte stride, 4-byte aligned); maxd2_dev: n f32
 * (4-byte aligned), the squared search radius of each point, or NULL = RT_T_MISS for every point ("however far");
 * out_dev: n x 32 B, 16-byte aligned; exactly 32 n bytes are written. All three are device memory on the renderer's GPU.
 * Asynchronous on the renderer's stream, exactly as rt_cast_rays is.
 * The answer, stated without a tree. Triangle j is its (a, e1, e2) record: a, e1 = b - a and e2 = c - a, the subtractions
 * in f32, as rt_set_bvh and rt_set_triangles_device keep it. One function of the point and that record gives (d2_j, v, w):
 * the nearest of five candidates — the nearest points of the edges ab, ac and bc, each by a clamped segment parameter,
 * and the projection onto the plane, as solved and after one refinement step, when it falls inside — in f32 with every operation rounded once in a fixed order, no
 * FMA, IEEE division, starting with p - a (a mesh far from the origin loses nothing); v >= 0, w >= 0 and v + w <= 1 hold
 * for every input, and d2_j is |(p - a) - (v e1 + w e2)|^2 evaluated for exactly those v, w (csrc/rt_closest.hpp is the
 * function; DESIGN.md §7e has its properties and its error bound). With cap = maxd2[i], or RT_T_MISS without maxd2,
 * record i holds the lexicographic minimum (d2_j, j) over the triangles with d2_j < cap, an f32 comparison: the smallest
 * squared distance, and among equal ones the smallest index; prim = j, v and w that triangle's, and p[k] = a[k] +
 * (v e1[k] + w e2[k]) rounded in that order. It is a miss when there is no such triangle.
 *   - A NaN d2_j is never accepted: a triangle with a non-finite a, e1 or e2 never answers, a non-finite point misses, and
 *     a distance whose square overflows (+inf) is below no cap.
 *   - A d2_j equal to the cap does not count. A NaN cap, or any cap <= 0 including -0, gives a miss; a cap above RT_T_MISS
 *     (+inf, FLT_MAX) behaves as RT_T_MISS. These are rt_occluded's tmax rules.
 *   - A zero-length edge or a zero-area triangle answers as the vertex or the edge it is: no NaN comes from finite input.
 * rt_host_closest_points is that sentence as a loop over every triangle, and the device returns its bytes: the tree only
 * skips triangles that cannot be accepted (a small cap skips most of the tree from the first node).
 * Programs and states: RT_ERR_ARG in the sphere program. The triangle and mixed programs need a triangle tree: device
 * geometry (rt_set_triangles_device, built or refitted) or rt_params.tri_bvh = 1 (the host SAH tree is built first if it
 * is not yet, as rt_get_tri_tree_cost does); RT_ERR_STATE without one, as rt_get_tri_tree_info. The spheres of the mixed
 * program are not part of the query: only triangles answer. A tree deeper than 24 (rt_get_tri_tree_info) can send points
 * to a slow, correct path, as it does rays.
 * n = 0 returns RT_OK and launches nothing. RT_ERR_ARG: n > 0 with a null points_dev or out_dev; a misaligned buffer. Like
 * the ray queries, it touches no image, frame count, stats, raw counters or learnt cost order. */
int rt_closest_points(rt_renderer *r, const void *points_dev, const void *maxd2_dev, uint32_t n, void *out_dev);
/* The definition on the host: pure CPU, no device. tris64: n_tris Triangle records (64 B each, as rt_set_bvh takes them;
 * no alignment asked); e1 = b - a and e2 = c - a are formed in f32 as the prep does. points: n x 3 f32; maxd2: n f32 or
 * NULL; out32: n rt_closest records (no alignment asked). RT_ERR_ARG: a null tris64 with n_tris > 0, or a null points or
 * out32 with n > 0. */
int rt_host_closest_points(const void *tris64, uint32_t n_tris, const float *points, const float *maxd2,
                           uint32_t n, void *out32);

/* Inside or outside: the generalized winding number of the triangle set at each of the caller's points (Jacobson et al.
 * 2013), w(p) = (1 / 4 pi) sum_j Omega_j(p) with Omega_j the signed solid angle of triangle j seen from p. 1 inside a
 * closed mesh wound outward (-1 for one wound inward), 0 outside, and in between where the mesh is open; cracks, holes
 * and overlapping shells do not break it, which ray parity and pseudo-normals cannot say of the (a, e1, e2) records kept
 * here. With rt_closest_points it gives a signed distance: negative where |w| >= 0.5.
 * points_dev: n x 3 f32, packed (12-byte stride, 4-byte aligned); w_dev: n f32 (4-byte aligned); exactly 4 n bytes are
 * written. Both are device memory on the renderer's GPU. Asynchronous on the renderer's stream, exactly as
 * rt_closest_points is.
 * beta is the far-field factor: 0 means the default 2.0; a value >= 1 is taken as it is; +inf sums every triangle of the
 * tree exactly, with no dipoles; NaN, a negative value or a value in (0, 1) is RT_ERR_ARG. A larger beta is more accurate
 * and slower (DESIGN.md §7f has measured errors: up to 0.04 to 0.07 at beta = 2 and 0.01 to 0.04 at beta = 3 on the project's
 * meshes, against 0.25 that the sign can bear).
 * The answer is a pure function of the tree bytes, the (a, e1, e2) records, the point and beta, and csrc/rt_winding.hpp is
 * that function for host and device alike (f32 triangle terms, one f64 accumulator per query, a written-out atan2, no
 * FMA, every operation rounded once in a fixed order):
 *   - the triangle term is Van Oosterom and Strackee's atan2 form on x0 = a - p, x1 = x0 + e1, x2 = x0 + e2, scaled by
 *     an exact power of two first; finite input never gives NaN or infinity; a triangle with a non-finite a, e1 or e2
 *     contributes 0;
 *   - per child of every node the tree carries two moments, the area-weighted normal sum N and the area-weighted centroid
 *     c (rt_host_tree_moments); a child whose c is further from the point than beta times the radius R of its box about
 *     c is taken whole as the dipole N . d / (4 L^3) (Barill et al. 2018, first order); otherwise a node child is
 *     descended and a leaf child's triangles are summed;
 *   - the flat definition — the triangle term over all triangles in index order, no dipoles — answers for a tree
 *     without nodes (four triangles or fewer), for a point outside the range the walk covers (rt_closest_points' D
 *     outside [2^-40, 2^60]) and for a query that overflows the walk's stack of 24 (a tree deeper than 24 can send
 *     points there, slow and correct);
 *   - a non-finite point gives the quiet NaN 0x7FC00000.
 * rt_host_winding_numbers is that function on the host, and the device returns its bytes for the same tree
 * (rt_host_lbvh_build_with gives the device builders' trees).
 * The moments are made by the first call after anything that changed the tree (rt_set_bvh, a device build or refit,
 * rt_release_scratch) and kept in device memory that rt_stats.device_bytes counts (64 B per node slot; rt_release_scratch frees it).
 * Programs and states are rt_closest_points': RT_ERR_ARG in the sphere program, for n > 0 with a null or misaligned
 * buffer, and for a bad beta; RT_ERR_STATE without a triangle tree (device geometry or rt_params.tri_bvh = 1; a host SAH
 * tree not built yet is built first). The spheres of the mixed program do not answer. n = 0 returns RT_OK and launches
 * nothing. It touches no image, frame count, stats, raw counters or learnt cost order. */
int rt_winding_numbers(rt_renderer *r, const void *points_dev, uint32_t n, float beta, void *w_dev);
/* The moments on the host: pure CPU, no device. tris64: n_tris Triangle records (64 B each; no alignment asked). hnodes,
 * node_slots, order, n_order, root_word and root (centre xyz, radius) are what rt_host_lbvh_build_with or
 * rt_testing_get_tri_tree return. moments_out: 64 B per node slot — per child {c[3] relative to the root centre, N[3], 0,
 * 0} as f32 —, the slots no child word names zero; moment_cap in slots. A tree without nodes (node_slots = 0) writes
 * nothing. RT_ERR_ARG: a null argument that is needed, moment_cap < node_slots, or bytes that are not a tree over order
 * and the triangles (a child word past node_slots or named twice, a leaf past n_order, an order entry past n_tris). */
int rt_host_tree_moments(const void *tris64, uint32_t n_tris, const void *hnodes, size_t node_slots,
                         const uint32_t *order, size_t n_order, uint32_t root_word, const float root[4],
                         void *moments_out, size_t moment_cap);
/* The query on the host: pure CPU, no device; the tree arguments as above. node_slots = 0 with a null hnodes gives the
 * flat definition (order, root_word and root are not read). points: n x 3 f32; w_out: n f32. RT_ERR_ARG as above, for a
 * bad beta, and for a null points or w_out with n > 0. */
int rt_host_winding_numbers(const void *tris64, uint32_t n_tris, const void *hnodes, size_t node_slots,
                            const uint32_t *order, size_t n_order, uint32_t root_word, const float root[4],
                            const float *points, uint32_t n, float beta, float *w_out);

/* Multi-hit ray queries (no reference counterpart): the k nearest triangles a ray passes through, in order, and the
 * number of all of them — what a loop of rt_cast_rays from hit to hit cannot give (it walks once per layer and drops the
 * second of two triangles hit at the same t). Triangle and mixed programs, on the triangle tree rt_closest_points walks.
 * origins_dev / dirs_dev as for rt_cast_rays; tmax_dev: n f32 or NULL (RT_T_MISS); after_dev: n rt_multi_hit records,
 * 4-byte aligned, of which only t and prim are read — a cursor per ray — or NULL; hits_dev: n x k records, 16-byte
 * aligned, ray i's record s at index i k + s, exactly 16 n k bytes written; counts_dev: n u32 or NULL. All device memory
 * on the renderer's GPU; asynchronous on the renderer's stream.
 *
 * The answer is stated without a tree (csrc/rt_multihit.hpp is the function, DESIGN.md section 7g the arguments). With rc
 * the root centre and rr_h the radius bound of the fp16 boxes that the other tree walks use, all in f32 with IEEE
 * division and square root and an FMA only where written:
 *   - op = o - rc, D = sqrt(op . op) * 1.001 + rr_h (the dot as (x x + y y) + z z), pad = D * 2^-12,
 *     inv_k = |d_k| >= 1e-30 ? 1 / d_k : copysign(1e30, d_k), c_lo_k = (-op_k - pad) * inv_k, c_hi_k = (-op_k + pad) * inv_k;
 *   - slab(box, upper): per axis t0 = fma(lo, inv, c_lo), t1 = fma(hi, inv, c_hi); enter = max(min(t0, t1) over the axes,
 *     0), exit = min(max(t0, t1) over the axes, upper), minimum and maximum as comparisons; hit when enter <= exit;
 *   - triangle j's own box: the f64 box of a, a + e1, a + e2 (e1 = b - a, e2 = c - a in f32; -0 as +0) rounded outward
 *     to f32 with one more ulp, each bound then (float)((double)v - (double)rc_k); a triangle with a non-finite a, e1 or
 *     e2 has no box;
 *   - triangle j is accepted when it has a box; the Moller-Trumbore test of rt_cast_rays' tree walk accepts it (the
 *     same operations in the same order: |det| >= 1e-4, 1 / det the IEEE division, 0 <= u <= 1, v >= 0, u + v <= 1, each
 *     dot as fma(az, bz, fma(ay, by, ax bx))); 1e-4 <= t_j < cap, where cap follows rt_occluded's tmax rules (NaN and
 *     everything <= 0: nothing; else min(tmax, RT_T_MISS)); (t_j, j) is lexicographically greater than the cursor's
 *     (t, prim) when a cursor is given; and slab(box_j, t_j) is hit — the computed t does not lie before the ray enters
 *     its own triangle's padded box.
 * Records 0 .. k-1 are the k smallest accepted (t_j, j) in ascending order with the test's own u, v (two triangles at
 * the same t are both listed, the smaller index first); unused records are the miss record {RT_T_MISS, -1, 0, 0};
 * counts[i] is the number of all accepted triangles, not capped by k. A ray with a non-finite component of o or d, or
 * a non-finite D, has no hits and count 0 (rt_cast_rays answers such a ray by the reference's rule instead: see there). The spheres of the mixed program do not answer.
 * Paging: each ray's last record of one call as the next call's cursor yields the next k hits; a miss record as cursor
 * yields nothing (nothing lies beyond RT_T_MISS), so any number of hits is reachable with k <= RT_MULTI_HIT_MAX_K.
 * rt_host_cast_rays_multi is that function on the host, and the device returns its bytes on every tree the renderer
 * holds, with or without counts (without them the walk culls by the list's last t; the records are the same). A query
 * that overflows the walk's stack of 24 runs the loop over all triangles instead.
 * Programs and states are rt_closest_points': RT_ERR_ARG in the sphere program, RT_ERR_STATE without a triangle tree
 * (device geometry or rt_params.tri_bvh = 1; a host SAH tree not built yet is built first). RT_ERR_ARG also for
 * k > RT_MULTI_HIT_MAX_K (for every n) and, with n > 0, for k = 0 without counts_dev, k > 0 without hits_dev, and a null
 * or misaligned buffer. n = 0 returns RT_OK and launches nothing, whatever the buffers and the program. It touches no image, frame count, stats, raw counters or learnt cost order. */
typedef struct rt_multi_hit { float t; int32_t prim; float u, v; } rt_multi_hit;   /* 16 B; miss: RT_T_MISS, -1, 0, 0 */
#define RT_MULTI_HIT_MAX_K 16u
int rt_cast_rays_multi(rt_renderer *r, const void *origins_dev, const void *dirs_dev, const void *tmax_dev,
                       const void *after_dev, uint32_t n, uint32_t k, void *hits_dev, void *counts_dev);
/* The query on the host: pure CPU, no device; the tree arguments as for rt_host_winding_numbers. node_slots = 0 with a
 * null hnodes gives the flat definition, a loop over all triangles in index order (order and root_word are not read);
 * root (centre xyz, radius) is always read: the constants above come from it. origins, dirs: n x 3 f32; tmax: n f32 or
 * NULL; after16: n records or NULL; hits16: n x k records; counts: n u32 or NULL (k = 0 needs it). RT_ERR_ARG: a null
 * argument that is needed, k > RT_MULTI_HIT_MAX_K, or bytes that are not a tree over order and the triangles. */
int rt_host_cast_rays_multi(const void *tris64, uint32_t n_tris, const void *hnodes, size_t node_slots,
                            const uint32_t *order, size_t n_order, uint32_t root_word, const float root[4],
                            const float *origins, const float *dirs, const float *tmax, const void *after16,
                            uint32_t n, uint32_t k, void *hits16, uint32_t *counts);

/* Volume queries (no reference counterpart): the triangles that touch an axis-aligned box, or the k nearest triangles of
 * a point within a radius, in order, and the number of all of them — the collision broad and narrow phase, voxelising a
 * mesh, neighbourhoods of a point, which one rt_closest_points record per point cannot give. Triangle and mixed programs,
 * on the triangle tree rt_closest_points walks. kind: RT_VOLUME_BOX or RT_VOLUME_BALL; volumes_dev: n queries packed as
 * the kind says, 4-byte aligned; after_dev: n rt_overlap_hit records, 4-byte aligned, of which only d2 and prim are read —
 * a cursor per query — or NULL; hits_dev: n x k records, 16-byte aligned, query i's record s at index i k + s, exactly
 * 16 n k bytes written; counts_dev: n u32 or NULL. All device memory on the renderer's GPU; asynchronous on the
 * renderer's stream.
 *
 * The answer is stated without a tree (csrc/rt_overlap.hpp is the function, DESIGN.md section 7h the arguments), over the
 * triangle records (a, e1 = b - a, e2 = c - a in f32) in index order, all in f32, every operation rounded once in the
 * order written, no FMA, with rc the root centre:
 *   - box (lo, hi): nothing for a non-finite bound or lo_k > hi_k on an axis. q_lo_k = the f32 at or below
 *     (double)lo_k - (double)rc_k, one more ulp down, q_hi_k likewise up; c_k = 0.5f lo_k + 0.5f hi_k,
 *     h_k = 0.5f hi_k - 0.5f lo_k; per triangle v0 = a - c, v1 = v0 + e1, v2 = v0 + e2, f0 = e1, f1 = e2 - e1, f2 = -e2.
 *     Triangle j is accepted when it has a box box_j (rt_cast_rays_multi's: none for a non-finite a, e1 or e2);
 *     q_lo_k <= box_j.hi_k && box_j.lo_k <= q_hi_k on all three axes; none of the nine axes unit_k x f_i separates — with
 *     k1 = (k + 1) % 3, k2 = (k + 2) % 3, a1 = -f_i[k2], a2 = f_i[k1]: p_m = a1 v_m[k1] + a2 v_m[k2] per vertex,
 *     r = h[k1] |a1| + h[k2] |a2|, separating when min(p) > r or max(p) < -r; and the plane axis n = e1 x e2 (each
 *     component as a product less a product) does not separate, with p_m = (n_x v_m.x + n_y v_m.y) + n_z v_m.z and
 *     r = (h_x |n_x| + h_y |n_y|) + h_z |n_z|. A comparison that fails, also one a NaN fails, does not separate: touching
 *     overlaps, and a degenerate triangle answers as the segment or point it is. Records {0.0f, j, 0, 0}, ascending in j.
 *   - ball (c, r2): cap follows rt_closest_points' maxd2 rules (NaN and everything <= 0: nothing; else min(r2,
 *     RT_T_MISS)); (d2_j, v, w) is rt_closest_points' point-triangle function of c and triangle j; accepted when
 *     d2_j < cap (equality does not count). Records {d2_j, j, v, w}, ascending in (d2, j). A non-finite c has no hits.
 *   - with a cursor a triangle is accepted only when (d2_j, j) — (0.0f, j) in the box kind — is lexicographically greater
 *     than the cursor's (d2, prim).
 * Records 0 .. k-1 are the first k accepted in that order; unused records are the miss record {RT_T_MISS, -1, 0, 0};
 * counts[i] is the number of all accepted triangles, not capped by k; a smaller k is a prefix of a larger one. The spheres
 * of the mixed program do not answer. Paging: each query's last record of one call as the next call's cursor yields the
 * next k; a miss record as cursor yields nothing.
 * rt_host_overlap_volumes is that function on the host, and the device returns its bytes on every tree the renderer holds,
 * with or without counts. A ball whose D = |c - rc| * 1.001 + rr_h lies outside [2^-40, 2^60], and a query that overflows
 * the walk's stack of 24, runs the loop over all triangles instead.
 * Programs and states are rt_cast_rays_multi's: RT_ERR_ARG in the sphere program, RT_ERR_STATE without a triangle tree
 * (device geometry or rt_params.tri_bvh = 1; a host SAH tree not built yet is built first). RT_ERR_ARG also for
 * k > RT_OVERLAP_MAX_K and for an unknown kind (for every n) and, with n > 0, for k = 0 without counts_dev, k > 0 without
 * hits_dev, and a null or misaligned buffer. n = 0 returns RT_OK and launches nothing, whatever the buffers and the
 * program. It touches no image, frame count, stats, raw counters or learnt cost order. */
#define RT_VOLUME_BOX   1u   /* volumes: n x 6 f32  {lo.x lo.y lo.z hi.x hi.y hi.z}              */
#define RT_VOLUME_BALL  2u   /* volumes: n x 4 f32  {c.x c.y c.z r2}  r2 = squared radius (a cap) */
#define RT_OVERLAP_MAX_K 16u
typedef struct rt_overlap_hit { float d2; int32_t prim; float v, w; } rt_overlap_hit;  /* 16 B; miss: RT_T_MISS, -1, 0, 0 */
int rt_overlap_volumes(rt_renderer *r, uint32_t kind, const void *volumes_dev, const void *after_dev,
                       uint32_t n, uint32_t k, void *hits_dev, void *counts_dev);
/* The query on the host: pure CPU, no device; the tree arguments as for rt_host_cast_rays_multi. node_slots = 0 with a
 * null hnodes gives the flat definition, a loop over all triangles in index order (order and root_word are not read);
 * root (centre xyz, radius) is always read. volumes: n x 6 or n x 4 f32; after16: n records or NULL; hits16: n x k
 * records; counts: n u32 or NULL (k = 0 needs it). RT_ERR_ARG: a null argument that is needed, k > RT_OVERLAP_MAX_K, an
 * unknown kind, or bytes that are not a tree over order and the triangles. */
int rt_host_overlap_volumes(const void *tris64, uint32_t n_tris, const void *hnodes, size_t node_slots,
                            const uint32_t *order, size_t n_order, uint32_t root_word, const float root[4],
                            uint32_t kind, const float *volumes, const void *after16,
                            uint32_t n, uint32_t k, void *hits16, uint32_t *counts);

/* Test-only entry points (fault injection) are declared in hrt_testing.h, not here: they are not part of
 * the drop-in surface. */

/* Raw per-draw device counters (no reference counterpart; diagnostics). Slots 0-4 are the rt_stats
 * work counters; in the diagnostic build (rt_diagnostic_build() == 1, lib/libhrt_diag.so) slots 8-11
 * hold summed wave clock cycles spent in closest-hit queries, shading, sample generation/accumulation
 * and whole wave lifetimes. Writes min(n, RT_RAW_COUNTERS) values, zero beyond. */
#define RT_RAW_COUNTERS 16
int rt_get_raw_counters(const rt_renderer *r, uint64_t *out, int n);
int rt_diagnostic_build(void);
/* Diagnostic build: per-wave records of the last launch of the last draw, 8 words per wave (waves in blockIdx.x *
 * waves per workgroup + wave order): start and end (s_memrealtime, 100 MHz ticks); HW_ID | XCC_ID << 32 (k_trace: the
 * longest time between two job takes in bits 0-23, its last job take << 40); the ticks until the wave first found no
 * work left | the frame blocks it generated << 32 (k_trace: the JOBS it took); the shader clock (s_memtime) at start,
 * end and that first drain; k_trace: lanes holding a sample at the drain | samples finished after the last job take
 * << 16 | rounds after the drain << 40 (scripts/wave_tail.py). Zero words in the product build. */
int rt_get_wave_trace(rt_renderer *r, uint64_t *out, size_t n_words);

/* Self-check of the kernels' range-restricted correctly rounded sqrt / division sequences against the IEEE
 * operations on n random cases each (diagnostics): mismatches[0] normalize of rng
 * vectors and normalize_exact of signed vectors, [1] division on [2^-60, 2^60] and the reciprocal of every
 * significand (case i's operand is fixed by i: n = 242 x 2^23 covers each under both signs of every binade
 * 2^-60 .. 2^60), [2] sqrt on [2^-100, 2^100].
 * All three must be 0. */
int rt_check_exact_math(uint64_t n, uint32_t seed, uint64_t mismatches[3]);

/* Self-check of the same sequences' range guards in their wave-uniform form (the fast sequence for every lane, one
 * __ballot deciding whether the wave recomputes its out-of-range lanes with the IEEE operation): the six inline helpers
 * the product kernels call, each called once per 64-lane wave on n_waves waves and compared bit for bit (NaNs too) with
 *   0 sqrt_exact_u       __builtin_sqrtf            3 div_by_radius3_u   x / radius per component
 *   1 normalize_exact_u  normalize                  4 div_by_len_rng_u   div_by_len_rng<false>
 *   2 candidate_t        exact_t_geo<false>, on the lanes sphere_candidate accepts (the others are passed need = false)
 *                                                   5 div_cam_u          x / l
 * Every lane holds operands inside the helper's fast range (edges included) and operands outside it, hashed from
 * (wave, lane, seed); the wave's pattern (wave index mod 8) picks the outside lanes at hashed positions: 0, 1, 31, 32, 63
 * or all 64 of a full wave; or a call inside a divergent branch with 1..63 lanes active, a hashed subset of them outside
 * (from none to all); or such a call whose only outside operands sit in the inactive lanes (the inactive lanes always
 * hold outside operands). Outside classes, drawn uniformly per lane:
 *   sqrt_exact_u      +0, a denormal, 2^-100 - 1 ulp, 2^100 + 1 ulp, +inf, a negative value, NaN
 *   normalize_exact_u a zero component, one at 2^-40 - 1 ulp, one at 2^40 + 1 ulp, all near 2^-80 (the dot underflows
 *                     to 0), all near 2^60, a NaN component; every sign
 *   candidate_t       the origin exactly on the sphere (integer coordinates: c == 0 and a zero numerator), disc below
 *                     2^-100, disc above 2^100 (r^2 = 2^102), 2a below 2^-60 (|d| near 2^-50), above 2^60 (|d| near
 *                     2^40), denormal (|d| near 2^-65), the numerator below 2^-60 and above 2^60
 *   div_by_radius3_u  inv_radius == 0 (radius outside [2^-60, 2^60]), a zero component, one below 2^-60, one above 2^60
 *   div_by_len_rng_u  both operands 0, both near 2^-60, a NaN operand
 *   div_cam_u         inv == 0 (l = 0 or outside [2^-60, 2^60]), x = 0, x below 2^-60, x above 2^60, NaN
 * out[helper * RT_UGUARD_WORDS + column], columns (lanes unless "calls"; "outside" by the check's own statement of the
 * documented range, not by reading the helper):
 *   0 mismatches (must be 0)   1 lanes compared   2 compared lanes outside the fast range
 *   3 of those, lanes where the fast sequence alone (no fallback) differs from the IEEE result: the lanes on which a
 *     fallback that did not run would show
 *   calls by their compared lanes outside the range: 4 none, 5 exactly one of several, 6 two or more but not all,
 *   7 every one   8 calls under a partial exec mask   9 candidate_t: outside lanes passed need = false
 * (diagnostics). */
#define RT_UGUARD_HELPERS 6u
#define RT_UGUARD_WORDS 10u
int rt_check_uniform_guards(uint64_t n_waves, uint32_t seed, uint64_t out[RT_UGUARD_HELPERS * RT_UGUARD_WORDS]);

/* The GPU a renderer draws on (no reference counterpart; the multi-GPU bench checks every rank's renderer against
 * its torch device): the HIP device ordinal that was current at rt_create, and that device's PCI location
 * {domain, bus, device}. A process must load ONE HIP runtime for the ordinal to mean what the caller's runtime
 * means (hrt/_lib.py loads the one torch uses). */
int rt_get_device(const rt_renderer *r, int32_t *ordinal, int32_t pci[3]);

/* ABI guard (no reference counterpart): rt_params and rt_stats grow at their ends between versions, and rt_set_params
 * / rt_get_stats copy this header's sizes. A caller built against another header checks *version == RT_ABI_VERSION (or
 * the two sizes against its own sizeof) before the first rt_set_params / rt_get_stats. Any pointer may be NULL. */
#define RT_ABI_VERSION 7u /* 7: rt_check_uniform_guards (no struct change); 6: rt_params.packet (round 6);
                             5: rt_params.cost_order, rt_stats.ordered_launches. rt_cast_rays / rt_primary_rays / rt_get_stream, then
                             rt_occluded, then rt_trace_rays / rt_primary_rng, then rt_bounce_rays, then rt_regroup_paths /
                             rt_host_regroup_keys, then rt_set_triangles_device / rt_host_lbvh_build, then
                             rt_refit_triangles_device / rt_host_lbvh_refit / rt_host_lbvh_cost / rt_get_tri_tree_cost, then
                             rt_set_triangles_device_with / rt_host_lbvh_build_with / rt_host_lbvh_refit_with /
                             rt_get_tri_tree_info, then rt_closest_points / rt_host_closest_points, then rt_winding_numbers /
                             rt_host_tree_moments / rt_host_winding_numbers, then rt_cast_rays_multi /
                             rt_host_cast_rays_multi, then rt_overlap_volumes / rt_host_overlap_volumes, came
                             later without a new version (no struct changed): detect them by their symbols */
int rt_abi_version(uint32_t *version, uint32_t *params_bytes, uint32_t *stats_bytes);

/* Thread-local message for the last failing call. */
const char *rt_last_error(void);
/* Number of visible gfx950 devices (0 on a CPU-only host; never an error). */
int rt_device_count(void);
/* Build string of the device code object ("gfx950 ..."), for the load check. */
const char *rt_build_info(void);

/* ================================ host-side scene builders ================================ */

/* Camera::new(from, to, focal_length, focal_blur_amount, fov) — src/scene/camera.rs:15-28 (glam 0.24 f32). */
int rt_host_camera_new(const float from[3], const float to[3], float focal_length, float focal_blur_amount,
                       float fov, void *camera80_out);

typedef struct rt_mesh rt_mesh;
typedef struct rt_tree rt_tree;

/* Mesh::load_obj(source, material) — src/geometry/mesh.rs:11-62 (tobj 4.0.3 default LoadOptions).
 * Like the reference, a parse failure yields an EMPTY mesh (status RT_OK) — see rt_host_mesh_counts. */
int rt_host_mesh_load_obj(const char *data, size_t len, const void *material32, rt_mesh **out);
int rt_host_mesh_counts(const rt_mesh *m, uint32_t *n_vertices, uint32_t *n_indices);
int rt_host_mesh_destroy(rt_mesh *m);

/* The size rules rt_set_bvh applies (sizes [n, m], buffer lengths, materials), without a device: RT_OK or
 * RT_ERR_ARG with rt_last_error() naming the rule. */
int rt_host_check_bvh_sizes(const uint32_t sizes[2], uint32_t n_nodes, uint32_t n_tris, uint32_t n_mats);

/* Tree::new / Tree::add_mesh / Tree::build — src/scene/bvh/tree.rs:20-90. */
int rt_host_tree_new(rt_tree **out);
int rt_host_tree_add_mesh(rt_tree *t, const rt_mesh *m);
int rt_host_tree_build(rt_tree *t);
/* Tree::build on `threads` host threads (0 = min(16, cores); rt_host_tree_build uses 0).
 * Level-synchronous BFS with concurrent stable sorts: byte-identical to the sequential build. */
int rt_host_tree_build_threads(rt_tree *t, int threads);
/* Views into the tree (valid until the next mutation): sizes [n, m], n nodes, m triangles, k materials. */
int rt_host_tree_view(const rt_tree *t, uint32_t sizes[2], const void **nodes32, uint32_t *n_nodes,
                      const void **tris64, uint32_t *n_tris, const void **mats32, uint32_t *n_mats);
int rt_host_tree_destroy(rt_tree *t);

/* render_ppm — src/scene/render_ppm.rs:38-57: ASCII P3, `(v*255) as u8` (saturating, truncating,
 * NaN -> 0). Writes at most cap bytes to out (may be NULL to query); *len = full length. */
int rt_host_render_ppm(const float *rgb, uint32_t width, uint32_t height, char *out, size_t cap, size_t *len);
/* compare_ppm_images — tests/rendering_tests.rs:84-131. Returns RT_OK if mean |du8| <= tolerance % of 255;
 * otherwise RT_ERR_COMPARE with *code = 1 DifferentDimensions, 2 PixelCountMismatch,
 * 3 ExcessiveDifference. *avg_diff_percent is filled whenever the pixel lists were compared. */
int rt_host_compare_ppm(const char *img1, size_t len1, const char *img2, size_t len2, float tolerance_percent,
                        int *code, float *avg_diff_percent);

#ifdef __cplusplus
}
#endif
#endif /* HRT_H */
