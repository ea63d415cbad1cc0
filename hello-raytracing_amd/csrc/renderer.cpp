// renderer.cpp — the rt_* C-ABI: device buffers, frame protocol and kernel launches on one HIP stream.
//
// Replaces the reference's wgpu Renderer (hucancode/hello-raytracing src/renderer.rs): the group0/group1
// bind-group buffers become device allocations owned by the handle, queue.write_buffer becomes a
// copy + layout conversion (AoS reference PODs -> the kernel's layout), and draw() becomes a kernel
// launch. There is no CPU fallback: without a gfx950 device every call that needs one returns
// RT_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../include/hrt.h"
#include "../../include/hrt_testing.h"
#include "host/scene.hpp"
#include "host/sphere_bvh.hpp"
#include "host/tri_bvh.hpp"
#include "rt_device.hpp"
#include "rt_closest.hpp"
#include "rt_lbvh.hpp"
#include "rt_regroup.hpp"
#include "rt_multihit.hpp"
#include "rt_overlap.hpp"
#include "rt_winding.hpp"
#include "rt_tile_lists.hpp"

hipError_t hrt_launch_render(int mode, int variant, const hrt_dev::KParams& P, hipStream_t stream);
hipError_t hrt_launch_accumulate(const hrt_dev::KParams& P, hipStream_t stream);
hipError_t hrt_launch_cast(int mode, int variant, const hrt_dev::KParams& P, const float* origins, const float* dirs, uint32_t n,
                           void* hits, hipStream_t stream);
hipError_t hrt_launch_occluded(int mode, int variant, const hrt_dev::KParams& P, const float* origins, const float* dirs,
                               const float* tmax, uint32_t n, void* occluded, hipStream_t stream);
hipError_t hrt_launch_trace_rays(int mode, int variant, const hrt_dev::KParams& P, const float* origins, const float* dirs,
                                 const uint32_t* rng, uint32_t seed, uint32_t n, uint32_t R, float* radiance, uint32_t* queries,
                                 hipStream_t stream);
hipError_t hrt_launch_bounce(int mode, int variant, const hrt_dev::KParams& P, const hrt_dev::BounceIO& io, uint32_t n,
                             hipStream_t stream);
hipError_t hrt_launch_primary_rays(int mode, const hrt_dev::KParams& P, uint32_t time, float* origins, float* dirs,
                                   uint32_t* state, hipStream_t stream);
hipError_t hrt_launch_regroup(const hrt_regroup::Launch& a, uint32_t n, hipStream_t stream);  // rt_regroup.hip
hipError_t hrt_launch_lbvh(const hrt_lbvh::Launch& a, hipStream_t stream);                     // rt_lbvh.hip
hipError_t hrt_launch_lbvh_refit(const hrt_lbvh::Refit& a, hipStream_t stream);                // rt_lbvh.hip
hipError_t hrt_launch_lbvh_ploc(const hrt_lbvh::Launch& a, uint64_t* pinned, hipStream_t stream);  // rt_ploc.hip
hipError_t hrt_launch_tri_tree_cost(const void* hnodes, uint32_t slots, uint32_t root, uint64_t* out, hipStream_t stream);  // rt_lbvh.hip
hipError_t hrt_launch_closest(const hrt_closest::Launch& a, bool count, hipStream_t stream);      // rt_closest.hip
hipError_t hrt_launch_winding(const hrt_winding::Launch& a, bool count, hipStream_t stream);      // rt_winding.hip
hipError_t hrt_launch_tree_moments(const hrt_winding::MomentsLaunch& a, hipStream_t stream);      // rt_winding.hip
hipError_t hrt_launch_multihit(const hrt_multihit::Launch& a, bool stats, hipStream_t stream);    // rt_multihit.hip
hipError_t hrt_launch_overlap(const hrt_overlap::Launch& a, bool stats, hipStream_t stream);      // rt_overlap.hip
hipError_t hrt_launch_trace(int mode, int variant, const hrt_dev::KParams& P, hipStream_t stream);
hipError_t hrt_launch_order(uint32_t* pixel_cost, uint32_t ntiles, uint32_t* tile_sum, uint32_t* order, uint32_t* scratch,
                            hipStream_t stream);
uint32_t hrt_order_scratch_words(uint32_t ntiles);
hipError_t hrt_launch_tile_lists(const hrt_tiles::View& V, const float4* bvh_sph, uint32_t nleaf, uint32_t* lists,
                                 hipStream_t stream);
const char* hrt_last_kernel();
void hrt_reset_last_kernel();
hipError_t hrt_check_exact_math(unsigned long long n, uint32_t seed, unsigned long long* out_dev, hipStream_t st);
hipError_t hrt_check_uniform_guards(unsigned long long n_waves, uint32_t seed, unsigned long long* out_dev, hipStream_t st);

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess)                                                                  \
            return fail(RT_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e_));    \
    } while (0)

template <typename T>
struct DevBuf {
    T* ptr = nullptr;
    size_t cap = 0;  // elements
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    uint64_t bytes() const { return ptr ? (uint64_t)cap * sizeof(T) : 0u; }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        cap = 0;
    }
};

// fail_above: fault injection for tests (rt_testing_set_faults), an allocation above that many bytes
// fails as a refused hipMalloc would (0 = off)
template <typename T>
int ensure(DevBuf<T>& b, size_t n, size_t fail_above = 0) {
    if (n <= b.cap && b.ptr) return RT_OK;
    b.release();
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    if (fail_above && bytes > fail_above)
        return fail(RT_ERR_ALLOC, "hipMalloc: injected failure (rt_testing_set_faults)");
    hipError_t e = hipMalloc((void**)&b.ptr, bytes);
    if (e != hipSuccess) {
        b.ptr = nullptr;
        return fail(RT_ERR_ALLOC, std::string("hipMalloc: ") + hipGetErrorString(e));
    }
    b.cap = std::max<size_t>(n, 1);
    return RT_OK;
}

// ensure() for the sample queue's colour-fold memory, which must stay within rt_params.queue_budget_mb: a buffer
// left larger by an earlier draw is given back when it exceeds `budget` bytes or twice what this draw needs.
template <typename T>
int ensure_within(DevBuf<T>& b, size_t n, size_t budget, size_t fail_above) {
    if (b.ptr && (b.cap * sizeof(T) > budget || b.cap > 2 * std::max<size_t>(n, 1))) b.release();
    return ensure(b, n, fail_above);
}

// Makes `device` current for one rt_* call and restores the caller's device after it: a renderer's memory, stream
// and launches stay on the GPU it was created on whatever device the calling thread has current (one process
// driving several GPUs, or a caller that switches devices between calls).
// prior: the status of a check made before it; when that failed nothing is done and rc is that status.
struct DeviceScope {
    int prev = -1, rc;
    explicit DeviceScope(int device, int prior = RT_OK) : rc(prior) {
        if (rc) return;
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) {
            rc = fail(RT_ERR_DEVICE, "hipGetDevice failed");
            return;
        }
        if (cur == device) return;
        if (hipSetDevice(device) != hipSuccess) {
            rc = fail(RT_ERR_DEVICE, "hipSetDevice to the renderer's device failed");
            return;
        }
        prev = cur;
    }
    ~DeviceScope() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope&) = delete;
    DeviceScope& operator=(const DeviceScope&) = delete;
};

// The counter words of one tree query's counting instantiation (include/hrt_testing.h): `on` selects it, the first
// counted call allocates the words.
struct CounterSlot {
    DevBuf<unsigned long long> buf;
    bool on = false;
    // Before a launch: *words = the `n` words, zeroed on `stream`, or null when counting is off.
    int arm(size_t n, hipStream_t stream, unsigned long long** words) {
        *words = nullptr;
        if (!on) return RT_OK;
        if (int rc = ensure(buf, n)) return rc;
        HIP_TRY(hipMemsetAsync(buf.ptr, 0, n * sizeof(unsigned long long), stream));
        *words = buf.ptr;
        return RT_OK;
    }
    // The `n` words of the last counted call (zeros before the first one). Blocking.
    int read(int device, hipStream_t stream, uint64_t* out, size_t n) const {
        std::fill(out, out + n, uint64_t{0});
        if (!buf.ptr) return RT_OK;
        DeviceScope ds(device);
        if (ds.rc) return ds.rc;
        HIP_TRY(hipMemcpyAsync(out, buf.ptr, n * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        return RT_OK;
    }
};

int check_device(int* dev_out) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(RT_ERR_DEVICE, "no HIP device visible (the renderer has no CPU fallback)");
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(RT_ERR_DEVICE, std::string("device is ") + prop.gcnArchName + ", this build targets gfx950 only");
    *dev_out = dev;
    return RT_OK;
}

// Rows owned by a renderer: blocks of `block` rows starting at row0, row0 + step*block, ... (block 1: the
// interleaved rows row0, row0 + step, ...); the last block may be cut by the image bottom.
uint32_t local_rows_of(uint32_t H, uint32_t row0, uint32_t step, uint32_t block) {
    if (row0 >= H || step == 0) return 0;
    block = std::max(block, 1u);
    const uint64_t stride = (uint64_t)step * block;
    const uint64_t nblocks = ((uint64_t)H - row0 + stride - 1) / stride;
    const uint64_t last0 = row0 + (nblocks - 1) * stride;  // first row of the last block
    return (uint32_t)((nblocks - 1) * block + std::min<uint64_t>(block, H - last0));
}

// The descent hold of k_trace_split<LNODES> (rt_kernels.hip bvh_walk_noovf<.., HOLD>): 0 = off. Not an rt_params field: a
// product caller has no use for it; hrt_testing.h moves it for the tests and the sweeps.
constexpr uint32_t DESCENT_HOLD_DEFAULT = 12u;

}  // namespace

struct rt_renderer {
    int device = 0;
    int mode = RT_MODE_SPHERE;
    uint32_t width = 0, height = 0;
    rt_params params{};
    hrt::Camera camera{};
    bool has_camera = false;
    uint32_t time = 0, frame_count = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;

    DevBuf<float> image;
    DevBuf<float4> sph_geo;
    DevBuf<hrt_dev::SphereAux> sph_aux;
    DevBuf<hrt_dev::SphereAux> code_aux;  // sph_aux in BVH-code order, then in slot order (KParams::code_aux)
    DevBuf<hrt_dev::SpherePair> sph_pairs;
    uint32_t n_spheres = 0;
    // culling BVH over the sphere slots (SCAN_BVH)
    DevBuf<float4> bvh_nodes, bvh_sph;
    DevBuf<uint4> bvh_hnodes;
    DevBuf<int> bvh_slot, bvh_large;
    hrt::SphereBvh bvh_host;
    DevBuf<float4> nodes;
    DevBuf<float> nodes_so;  // the same nodes as (lo, hi, lo) per axis (pack_nodes_so)
    bool so_ok = false;
    DevBuf<hrt_dev::TriDev> tris;
    DevBuf<float> tri_geo;  // a | e1 | e2 per triangle, 9 floats (the deferred tests' operands; KParams::tri_geo)
    DevBuf<hrt_dev::MatDev> mats;
    uint32_t bvh_n = 0, bvh_m = 0;
    // opt-in SAH triangle tree, built on first use after rt_set_bvh
    std::vector<float> tri_aee;  // a, e1, e2 of every triangle as uploaded
    bool tri_tree_dirty = true;
    hrt::TriBvh tri_tree;
    DevBuf<uint4> tb_hnodes;
    DevBuf<uint32_t> tb_order;
    // device geometry only: the parent links of the tree in tb_hnodes (rt_lbvh.hpp Launch::parent, for the bvh_m triangles
    // it was built over). Part of the tree, not scratch: rt_refit_triangles_device climbs them.
    DevBuf<uint32_t> tb_parent;
    uint32_t tb_n_nodes = 0, tb_n_order = 0;  // nodes (2 uint4 each) and leaf positions the two buffers hold
    // device geometry only (rt_get_tri_tree_info): the builder of the tree in tb_hnodes, and PLOC's iteration counts
    uint32_t tb_builder = RT_TREE_LBVH, tb_iterations = 0, tb_flat = 0;
    // rt_set_triangles_device: true = device geometry (tris, tri_geo and the tree were made on the device: there is no
    // reference heap and no tri_aee, and every draw and query walks the tree whatever rt_params.tri_bvh says; tri_tree
    // holds only the root word, centre, radius and depth). rt_set_bvh leaves the state.
    bool dev_geom = false;
    uint32_t dev_n_mats = 0;  // the materials the device geometry came with (a refit checks the indices against it)
    // its staging buffers (a build writes these; success swaps them with tris, tri_geo, mats, tb_hnodes, tb_order and
    // tb_parent (lb_parent is the staging copy of the links); a refit swaps tris, tri_geo and tb_hnodes alone, so
    // they then hold the geometry before: two sets that alternate for a mesh that moves every step) and its scratch
    // (rt_lbvh.hpp Launch): keys and sorted keys, parent links, arrival counters, box slots, the status block
    DevBuf<hrt_dev::TriDev> lb_tris;
    DevBuf<float> lb_geo;
    DevBuf<hrt_dev::MatDev> lb_mats;
    DevBuf<uint4> lb_hnodes;
    DevBuf<uint32_t> lb_order, lb_keys, lb_parent, lb_arrivals;
    DevBuf<uint64_t> lb_boxes, lb_stat;
    // pinned: the status read-backs of the refit and of the PLOC build land here (allocated by the first of them)
    uint64_t* refit_stat_host = nullptr;
    DevBuf<unsigned long long> counter;
    DevBuf<unsigned long long> count_spread;  // the work counters' CSPREAD copies (rt_kernels.hip flush_counts)
    DevBuf<unsigned long long> steal_slots;  // sample queue: one word per resident wave (frame-block work stealing)
    DevBuf<unsigned long long> queues;       // sample buffer: the per-XCD job counters (rt_kernels.hip queue_take_lane0)
    uint32_t cus = 0;                        // compute units of the renderer's device
    DevBuf<float> samples;      // sample-queue colour buffer (frames x tiles x 64 px x 3), tile-major (ring_mode 0)
    DevBuf<float> samples2;     // the odd launches' buffer when each launch folds the one before (rt_params.fold 3)
    bool last_fold_next = false;
    DevBuf<float4> ring;        // sample-queue fold ring: job slots x job_frames x 64 px (rgb, unused) (ring_mode 1)
    DevBuf<uint32_t> ring_ctl;  // zeroed per launch: tile fold words (2 words per tile), the free queue (4 per
                                // slot) and its tail (4); then the job -> slot map
    // cost-ordered dealing (rt_params.cost_order): per-pixel query counts of a learning launch (zeroed again by the
    // sort), per-tile sums, the tile order built from them, the counting sort's histogram / cursors; cost_tiles: the
    // tile count they were set up for, order_tiles: the tile count tile_order holds a permutation of (0: none yet);
    // cost_learn: the next sample-buffer launch learns (set by every scene, camera, size or parameter change)
    DevBuf<uint32_t> tile_cost, tile_sum, tile_order, order_scratch;
    uint32_t cost_tiles = 0, order_tiles = 0;
    // the tiles' primary candidate lists (rt_tile_lists.hpp; KParams::tile_lists): built by the first draw that can use
    // them and again whenever the view they were built for (camera, image, row share, K) or the sphere set differs;
    // tile_list_mode / _k: hrt_testing.h (0 auto = on, 1 off, 2 on)
    DevBuf<uint32_t> tile_lists;
    hrt_tiles::View tile_view{};
    bool tile_lists_valid = false;
    unsigned long long blocks_resolved = 0;  // of the last draw whose statistics were read (finish_stats)
    uint32_t tile_list_mode = 0, tile_list_k = hrt_tiles::K_MAX;
    bool cost_learn = true;
    uint32_t last_ordered = 0;  // trace launches of the last sample-queue draw that dealt in cost order
    DevBuf<unsigned long long> wave_trace;  // diagnostic build only
    size_t wave_trace_words = 0;
    // rt_regroup_paths' sort: 4 u32 per entry, and the digit counts (rt_regroup.hpp Launch; include/hrt.h has the size rule)
    DevBuf<uint32_t> regroup_entries, regroup_counts;
    // the counting instantiations of rt_closest_points (4 words), rt_winding_numbers (5), rt_cast_rays_multi (4) and
    // rt_overlap_volumes (4) (hrt_testing.h)
    CounterSlot closest_count, winding_count, multihit_count, overlap_count;
    // rt_winding_numbers: the moments of the tree in tb_hnodes (rt_winding.hpp: 16 floats per node slot), made by the first
    // call after anything that changed the tree (moments_dirty)
    DevBuf<float> tb_moments;
    bool moments_dirty = true;

    // host copy of the spheres (slot arrays are rebuilt when min_sphere_slots changes)
    std::vector<hrt::Sphere> spheres;

    rt_stats stats{};
    bool timing_pending = false;
    int last_variant = 0;
    std::vector<hipEvent_t> ev_trace;  // start/stop pairs around each k_trace launch of the last draw
    uint32_t trace_pairs = 0, trace_pairs_pending = 0;
    uint32_t last_schedule = 0;
    uint32_t last_suspend = 0;
    uint32_t test_ring_slots_max = 0, test_fail_alloc_above_mb = 0;  // hrt_testing.h fault injection
    uint32_t trace_rays_per_lane = 0;  // k_radiance_rays' R forced (hrt_testing.h); 0 = the rule (trace_rays_per_lane())
    uint32_t descent_hold = DESCENT_HOLD_DEFAULT;  // k_trace_split<LNODES>'s descent hold (hrt_testing.h moves it)
    uint32_t ring_slots = 0;  // fold-ring slots of the last sample-queue draw
    uint32_t ring_tiles = 0, ring_nchunks = 0;  // (diagnostics: HRT_RING_DUMP)
    size_t ring_ctl_words = 0;
    uint64_t fold_bytes = 0;  // device memory of the last sample-queue draw's colour fold (rt_stats.fold_bytes)
    uint32_t last_launch_frames = 0;  // frames per trace launch of the last sample-queue draw (rt_stats.launch_frames)
    unsigned long long raw_counters[RT_RAW_COUNTERS] = {};

    uint32_t row_block() const { return std::max(params.row_block, 1u); }
    uint64_t device_bytes() const {
        return image.bytes() + sph_geo.bytes() + sph_aux.bytes() + code_aux.bytes() + sph_pairs.bytes() + bvh_nodes.bytes() +
               bvh_sph.bytes() +
               bvh_hnodes.bytes() + bvh_slot.bytes() + bvh_large.bytes() + nodes.bytes() + nodes_so.bytes() + tris.bytes() +
               tri_geo.bytes() + mats.bytes() +
               tb_hnodes.bytes() + tb_order.bytes() + tb_parent.bytes() + counter.bytes() + count_spread.bytes() + samples.bytes() + samples2.bytes() + ring.bytes() + ring_ctl.bytes() +
               wave_trace.bytes() + steal_slots.bytes() + queues.bytes() + tile_cost.bytes() + tile_sum.bytes() + tile_order.bytes() +
               order_scratch.bytes() + tile_lists.bytes() + regroup_entries.bytes() + regroup_counts.bytes() + closest_count.buf.bytes() + tb_moments.bytes() + winding_count.buf.bytes() + multihit_count.buf.bytes() + overlap_count.buf.bytes() + lb_tris.bytes() + lb_geo.bytes() +
               lb_mats.bytes() + lb_hnodes.bytes() + lb_order.bytes() + lb_keys.bytes() + lb_parent.bytes() +
               lb_arrivals.bytes() + lb_boxes.bytes() + lb_stat.bytes();
    }
    uint32_t local_rows() const { return local_rows_of(height, params.row0, params.row_step, row_block()); }
    size_t image_floats() const { return (size_t)local_rows() * width * 3u; }
};

// heap-top configuration of k_trace_split_tris when rt_params.heap_lds = 0 (rt_kernels.hip heap_top_n)
constexpr uint32_t HEAP_AUTO = 3u;

namespace {

// The dielectric scatter arm's per-hit divisions, done once per material with the kernels' f32 operations
// (shader_sphere.wgsl:185-199: ir = 1 / params.x on a front face; reflectance's r0 = (1 - ir) / (1 + ir)).
hrt_dev::DielConsts dielectric_consts(float param) {
    auto r0sq = [](float ir) {
        const float r0 = (1.0f - ir) / (1.0f + ir);
        return r0 * r0;
    };
    const float inv = 1.0f / param;
    return hrt_dev::DielConsts{inv, r0sq(inv), r0sq(param)};
}

// rt_set_bvh's and rt_set_triangles_device's materials as the kernels read them.
std::vector<hrt_dev::MatDev> pack_materials(const void* mats32, uint32_t n_mats) {
    const hrt::Material* M = (const hrt::Material*)mats32;
    std::vector<hrt_dev::MatDev> md(n_mats);
    for (uint32_t k = 0; k < n_mats; k++) {
        const hrt_dev::DielConsts dc = dielectric_consts(M[k].params.x);
        md[k] = hrt_dev::MatDev{M[k].albedo.x, M[k].albedo.y, M[k].albedo.z, M[k].params.x, M[k].kind,
                                dc.inv_param, dc.r0sq_front, dc.r0sq_back};
    }
    return md;
}

int zero_image(rt_renderer* r) {
    int rc = ensure(r->image, r->image_floats());
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(r->image.ptr, 0, std::max<size_t>(r->image_floats(), 1) * sizeof(float), r->stream));
    return RT_OK;
}

// Nodes of a two-child BVH as the kernels read them: 4 float4 per node, boxes relative to `center`,
// rounded outward again after the shift.
std::vector<float4> pack_bvh_nodes(const std::vector<hrt::SphereBvhNode>& nodes, const float center[3]) {
    std::vector<float4> out(4 * std::max<size_t>(nodes.size(), 1));
    auto rel_lo = [&](float v, int k) { return std::nextafter((float)((double)v - (double)center[k]), -INFINITY); };
    auto rel_hi = [&](float v, int k) { return std::nextafter((float)((double)v - (double)center[k]), INFINITY); };
    for (size_t j = 0; j < nodes.size(); j++) {
        const hrt::SphereBvhNode& n = nodes[j];
        float4* o = &out[4 * j];
        o[0] = float4{rel_lo(n.lmin[0], 0), rel_lo(n.lmin[1], 1), rel_lo(n.lmin[2], 2), __builtin_bit_cast(float, n.left)};
        o[1] = float4{rel_hi(n.lmax[0], 0), rel_hi(n.lmax[1], 1), rel_hi(n.lmax[2], 2), 0.0f};
        o[2] = float4{rel_lo(n.rmin[0], 0), rel_lo(n.rmin[1], 1), rel_lo(n.rmin[2], 2), __builtin_bit_cast(float, n.right)};
        o[3] = float4{rel_hi(n.rmax[0], 0), rel_hi(n.rmax[1], 1), rel_hi(n.rmax[2], 2), 0.0f};
    }
    return out;
}

// The heap's nodes for the sign-ordered node test (rt_kernels.hip node_hit_so; tests/test_sign_ordered_slab.py):
// (lo, hi, lo) per axis, 9 floats per node, with lo <= hi — an axis with min > max (padding nodes: +MAX / -MAX) is
// swapped, which changes nothing in intersect_node (shader_tris.wgsl:150-159: min / max take the pair in either order).
// A NaN bound leaves its axis as given and clears so_ok (the kernels then use the reference form on this layout).
std::vector<float> pack_nodes_so(const float* nodes, uint32_t n, bool& so_ok) {
    std::vector<float> out(9 * (size_t)std::max<uint32_t>(n, 1), 0.0f);
    so_ok = true;
    for (uint32_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) {
            float lo = nodes[8 * (size_t)i + k], hi = nodes[8 * (size_t)i + 4 + k];
            if (std::isnan(lo) || std::isnan(hi)) so_ok = false;
            else if (lo > hi) std::swap(lo, hi);
            out[9 * (size_t)i + 3 * k] = lo;
            out[9 * (size_t)i + 3 * k + 1] = hi;
            out[9 * (size_t)i + 3 * k + 2] = lo;
        }
    }
    return out;
}

// The culling BVH's nodes with fp16 boxes (k_trace_split): 32 B per node instead of 64 — per child the
// box relative to `center` as six halves rounded outward (min down, max up: containment holds, so the walk
// stays exact; the boxes only grow by at most one half ulp), then the child word:
//   (min.x | min.y << 16, min.z | max.x << 16, max.y | max.z << 16, left word), the same for the right.
// (f16_dir: rt_lbvh.hpp, shared with the device-built triangle tree)
using hrt_lbvh::f16_dir;
std::vector<uint4> pack_bvh_hnodes(const std::vector<hrt::SphereBvhNode>& nodes, const float center[3]) {
    std::vector<uint4> out(2 * std::max<size_t>(nodes.size(), 1), uint4{0u, 0u, 0u, 0u});
    auto rel = [&](float v, int k, bool up) {
        const float f = std::nextafter((float)((double)v - (double)center[k]), up ? INFINITY : -INFINITY);
        return f16_dir(f, up);
    };
    for (size_t j = 0; j < nodes.size(); j++) {
        const hrt::SphereBvhNode& n = nodes[j];
        const float* mn[2] = {n.lmin, n.rmin};
        const float* mx[2] = {n.lmax, n.rmax};
        const uint32_t w[2] = {n.left, n.right};
        for (int c = 0; c < 2; c++) {
            // per axis one [min | max] pair of halves (k_trace_split rotates a pair to [near | far]: box_hit_so)
            out[2 * j + c] = uint4{rel(mn[c][0], 0, false) | rel(mx[c][0], 0, true) << 16,
                                   rel(mn[c][1], 1, false) | rel(mx[c][1], 1, true) << 16,
                                   rel(mn[c][2], 2, false) | rel(mx[c][2], 2, true) << 16, w[c]};
        }
    }
    return out;
}

int upload_tri_tree(rt_renderer* r) {
    if (r->dev_geom || !r->tri_tree_dirty) return RT_OK;  // (device geometry: the tree is there, and tri_aee is not)
    r->tri_tree = hrt::build_tri_bvh(r->tri_aee);
    const std::vector<uint4> hpacked = pack_bvh_hnodes(r->tri_tree.nodes, r->tri_tree.root_center);
    int rc = ensure(r->tb_hnodes, hpacked.size());
    if (!rc) rc = ensure(r->tb_order, std::max<size_t>(r->tri_tree.order.size(), 1));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(r->tb_hnodes.ptr, hpacked.data(), hpacked.size() * sizeof(uint4), hipMemcpyHostToDevice,
                           r->stream));
    if (!r->tri_tree.order.empty())
        HIP_TRY(hipMemcpyAsync(r->tb_order.ptr, r->tri_tree.order.data(), r->tri_tree.order.size() * sizeof(uint32_t),
                               hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->tb_n_nodes = (uint32_t)r->tri_tree.nodes.size();
    r->tb_n_order = (uint32_t)r->tri_tree.order.size();
    r->tri_tree_dirty = false;
    r->moments_dirty = true;
    return RT_OK;
}

template <typename T>
void swap_buffers(DevBuf<T>& a, DevBuf<T>& b) {
    std::swap(a.ptr, b.ptr);
    std::swap(a.cap, b.cap);
}

int upload_spheres(rt_renderer* r) {
    const uint32_t nslots = std::max<uint32_t>((uint32_t)r->spheres.size(), r->params.min_sphere_slots);
    std::vector<float4> geo(nslots, float4{0.0f, 0.0f, 0.0f, 0.0f});
    std::vector<hrt_dev::SphereAux> aux(nslots);
    std::memset(aux.data(), 0, aux.size() * sizeof(aux[0]));
    for (uint32_t i = (uint32_t)r->spheres.size(); i < nslots; i++) {  // zero slots: params 0, id 0 (default arm)
        const hrt_dev::DielConsts dc = dielectric_consts(0.0f);
        aux[i].inv_param = dc.inv_param;
        aux[i].r0sq_front = dc.r0sq_front;
        aux[i].r0sq_back = dc.r0sq_back;
    }
    for (size_t i = 0; i < r->spheres.size(); i++) {
        const hrt::Sphere& s = r->spheres[i];
        const float rr = s.radius * s.radius;  // radius*radius, shader_sphere.wgsl:142
        geo[i] = float4{s.center.x, s.center.y, s.center.z, rr};
        const hrt_dev::DielConsts dc = dielectric_consts(s.material.params.x);
        const bool rad_ok = std::fabs(s.radius) >= 0x1p-60f && std::fabs(s.radius) <= 0x1p60f;
        aux[i] = hrt_dev::SphereAux{s.center.x, s.center.y, s.center.z, s.radius,
                                    s.material.albedo.x, s.material.albedo.y, s.material.albedo.z,
                                    s.material.params.x, s.material.kind, dc.inv_param, dc.r0sq_front, dc.r0sq_back,
                                    rad_ok ? 1.0f / s.radius : 0.0f, 0.0f, 0.0f, 0.0f};
    }
    // slot pairs for the packed scan; an odd tail slot is paired with a NaN-centre slot (never accepted)
    const uint32_t npairs = (nslots + 1) / 2;
    const float qnan = std::nanf("");
    std::vector<hrt_dev::SpherePair> pairs(npairs);
    for (uint32_t p = 0; p < npairs; p++) {
        for (int k = 0; k < 2; k++) {
            const uint32_t i = 2 * p + (uint32_t)k;
            const float4 g = i < nslots ? geo[i] : float4{qnan, qnan, qnan, 0.0f};
            pairs[p].cx[k] = g.x;
            pairs[p].cy[k] = g.y;
            pairs[p].cz[k] = g.z;
            pairs[p].rr[k] = g.w;
        }
    }
    // culling BVH: boxes stored relative to the root centre (rounded outward again after the shift)
    std::vector<float> cr(4 * (size_t)nslots);
    for (uint32_t i = 0; i < nslots; i++) {
        const bool real = i < r->spheres.size();
        cr[4 * i + 0] = geo[i].x;
        cr[4 * i + 1] = geo[i].y;
        cr[4 * i + 2] = geo[i].z;
        cr[4 * i + 3] = real ? r->spheres[i].radius : 0.0f;
    }
    r->bvh_host = hrt::build_sphere_bvh(cr);
    const hrt::SphereBvh& B = r->bvh_host;
    const std::vector<float4> bnodes = pack_bvh_nodes(B.nodes, B.root_center);
    const std::vector<uint4> hnodes = pack_bvh_hnodes(B.nodes, B.root_center);
    const size_t nleaf = B.slot.size();
    // the hit records in BVH-code order (leaf positions, then the large list), then in slot order: k_trace_split
    // shades its winner by code, and the full-scan fallback's slot indexes the tail (KParams::code_aux)
    std::vector<hrt_dev::SphereAux> caux;
    caux.reserve(nleaf + B.large.size() + nslots);
    for (const int sl : B.slot) caux.push_back(aux[(size_t)sl]);
    for (const int sl : B.large) caux.push_back(aux[(size_t)sl]);
    caux.insert(caux.end(), aux.begin(), aux.end());
    // (k_trace_split reads the table through a buffer descriptor: a 32-bit range, KParams::code_aux_bytes)
    if (caux.size() * sizeof(caux[0]) > 0xFFFFFFFFull) return fail(RT_ERR_ARG, "too many sphere slots for the hit-record table");
    int rc = ensure(r->sph_geo, nslots);
    if (!rc) rc = ensure(r->sph_aux, nslots);
    if (!rc) rc = ensure(r->code_aux, std::max<size_t>(caux.size(), 1));
    if (!rc) rc = ensure(r->sph_pairs, npairs);
    if (!rc) rc = ensure(r->bvh_nodes, bnodes.size());
    if (!rc) rc = ensure(r->bvh_hnodes, hnodes.size());
    if (!rc) rc = ensure(r->bvh_sph, std::max<size_t>(nleaf, 1));
    if (!rc) rc = ensure(r->bvh_slot, std::max<size_t>(nleaf, 1));
    if (!rc) rc = ensure(r->bvh_large, std::max<size_t>(B.large.size(), 1));
    if (rc) return rc;
    if (nslots) {
        HIP_TRY(hipMemcpyAsync(r->sph_geo.ptr, geo.data(), nslots * sizeof(float4), hipMemcpyHostToDevice, r->stream));
        HIP_TRY(hipMemcpyAsync(r->sph_aux.ptr, aux.data(), nslots * sizeof(aux[0]), hipMemcpyHostToDevice, r->stream));
        HIP_TRY(hipMemcpyAsync(r->code_aux.ptr, caux.data(), caux.size() * sizeof(caux[0]), hipMemcpyHostToDevice,
                               r->stream));
        HIP_TRY(hipMemcpyAsync(r->sph_pairs.ptr, pairs.data(), npairs * sizeof(pairs[0]), hipMemcpyHostToDevice,
                               r->stream));
        HIP_TRY(hipMemcpyAsync(r->bvh_nodes.ptr, bnodes.data(), bnodes.size() * sizeof(float4),
                               hipMemcpyHostToDevice, r->stream));
        HIP_TRY(hipMemcpyAsync(r->bvh_hnodes.ptr, hnodes.data(), hnodes.size() * sizeof(uint4),
                               hipMemcpyHostToDevice, r->stream));
        if (nleaf) {
            HIP_TRY(hipMemcpyAsync(r->bvh_sph.ptr, B.sph.data(), nleaf * sizeof(float4), hipMemcpyHostToDevice,
                                   r->stream));
            HIP_TRY(hipMemcpyAsync(r->bvh_slot.ptr, B.slot.data(), nleaf * sizeof(int), hipMemcpyHostToDevice,
                                   r->stream));
        }
        if (!B.large.empty())
            HIP_TRY(hipMemcpyAsync(r->bvh_large.ptr, B.large.data(), B.large.size() * sizeof(int),
                                   hipMemcpyHostToDevice, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));  // host staging vectors die here
    }
    r->n_spheres = nslots;
    r->tile_lists_valid = false;
    return RT_OK;
}

// Event pairs for `pairs + 1` k_trace launches (created on demand, kept for the renderer's life).
int trace_events(rt_renderer* r, uint32_t pair) {
    while (r->ev_trace.size() < 2u * (pair + 1u)) {
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        r->ev_trace.push_back(e);
    }
    return RT_OK;
}

// schedule 0 = the sample queue (load-balanced at sample granularity), except for
// draws too small to fill the persistent grid for long (< 1.5 Mi samples: e.g. a 512x512 interactive
// frame, C1), where the tiles kernel's single launch has less fixed cost. Measured per step (ms, tiles vs
// queue): C1 0.13 vs 0.16; 512x512 x1 0.22 vs 0.29; C2 x2 frames (1.8 M) 0.54 vs 0.50; one 1080p frame
// of C3 (2.1 M) 1.55 vs 1.33.
uint32_t resolve_schedule(const rt_renderer* r, uint32_t count) {
    if (r->params.schedule) return r->params.schedule;
    const uint64_t samples = (uint64_t)count * r->local_rows() * r->width;
    return samples < (3ull << 19) ? RT_SCHEDULE_TILES : RT_SCHEDULE_QUEUE;
}

// variant 0 = the fastest exact scan measured for the slot count: the culling BVH from 32 slots up, the
// deferred packed scan from 9, the simple scan below (C2, 4 slots: 50.8 vs 48.0 Grays/s deferred).
int resolve_variant(const rt_renderer* r) {
    if (r->params.variant) return (int)r->params.variant;
    if (r->n_spheres >= 32) return hrt_dev::SCAN_BVH;
    return r->n_spheres > 8 ? hrt_dev::SCAN_DEFER : hrt_dev::SCAN_SIMPLE;
}

// The scene and camera part of the kernel arguments, shared by the draws (launch_frames) and the ray queries
// (rt_cast_rays, rt_primary_rays): camera constants, row partition, sphere slots with their culling BVH, the triangle
// heap and, with tri_bvh, the SAH tree. Uploads what is still missing (the zero slots of an empty sphere scene, the SAH
// tree on its first use). P arrives zeroed; what only a draw reads or writes (frames, bounces, image, counters,
// schedule) is the caller's. Without a camera (a cast needs none) P.cam stays zero.
int scene_params(rt_renderer* r, hrt_dev::KParams& P) {
    if (r->mode == RT_MODE_SPHERE && r->sph_geo.ptr == nullptr) {
        int rc = upload_spheres(r);  // empty scene: min_sphere_slots zero slots, like an unwritten buffer
        if (rc) return rc;
    }
    if (r->has_camera) {
        hrt_dev::CamDev& cd = P.cam;
        const hrt::Camera& c = r->camera;
        const float* cam = &c.eye.x;
        for (int i = 0; i < 4; i++) {
            cd.eye[i] = cam[i];
            cd.dir[i] = cam[4 + i];
            cd.up[i] = cam[8 + i];
            cd.right[i] = cam[12 + i];
        }
        cd.focal = c.params.x;
        cd.blur = c.params.y;
        cd.k = std::tan(c.params.z * 0.5f);  // tan(camera.fov*0.5), make_ray :124 (libm tanf, as the oracle)
        cd.aspect = (float)r->width / (float)r->height;
        cd.wm1 = (float)r->width - 1.0f;
        cd.hm1 = (float)r->height - 1.0f;
        // for the fast exact divisions of make_ray's px / wm1, py / hm1 (div_rn_mid's operand range)
        const auto inv_in_range = [](float l) { return l >= 0x1p-60f && l <= 0x1p60f ? 1.0f / l : 0.0f; };
        cd.inv_wm1 = inv_in_range(cd.wm1);
        cd.inv_hm1 = inv_in_range(cd.hm1);
        cd.H = r->height;
    }
    P.W = r->width;
    P.H = r->height;
    P.nslots = r->mode == RT_MODE_TRIS ? 0u : r->n_spheres;
    P.npairs = (P.nslots + 1) / 2;
    P.sph_pairs = r->sph_pairs.ptr;
    P.n = r->mode == RT_MODE_SPHERE ? 0u : r->bvh_n;
    P.m = r->mode == RT_MODE_SPHERE ? 0u : r->bvh_m;
    P.row0 = r->params.row0;
    P.row_step = r->params.row_step;
    P.row_block = r->row_block();
    P.row_stride = r->params.row_step * P.row_block;
    P.nrows = r->local_rows();
    P.sph_geo = r->sph_geo.ptr;
    P.sph_aux = r->sph_aux.ptr;
    P.code_aux = r->code_aux.ptr;
    P.nodes = r->nodes.ptr;
    P.nodes_so = r->nodes_so.ptr;
    P.so_ok = r->so_ok ? 1u : 0u;
    P.tris = r->tris.ptr;
    P.tri_geo = r->tri_geo.ptr;
    P.tri_bvh = (r->mode != RT_MODE_SPHERE && (r->params.tri_bvh || r->dev_geom)) ? 1u : 0u;
    if (P.tri_bvh) {
        int rc = upload_tri_tree(r);
        if (rc) return rc;
        P.tb_hnodes = r->tb_hnodes.ptr;
        P.tb_rr_h = std::nextafter(r->tri_tree.root_radius * (1.0f + 0x1p-9f), INFINITY);
        P.tb_order = r->tb_order.ptr;
        P.tb_root = r->tri_tree.root_word;
        for (int k = 0; k < 3; k++) P.tb_rc[k] = r->tri_tree.root_center[k];
        P.tb_rr = r->tri_tree.root_radius;
    }
    P.mats = r->mats.ptr;
    const hrt::SphereBvh& B = r->bvh_host;
    P.bvh_nodes = r->bvh_nodes.ptr;
    P.bvh_sph = r->bvh_sph.ptr;
    P.bvh_slot = r->bvh_slot.ptr;
    P.large_slots = r->bvh_large.ptr;
    P.nlarge = (uint32_t)B.large.size();
    P.bvh_nleaf = (uint32_t)B.slot.size();
    P.bvh_root = B.root_word;
    for (int k = 0; k < 3; k++) P.bvh_rc[k] = B.root_center[k];
    P.bvh_rr = B.root_radius;
    P.bvh_hnodes = r->bvh_hnodes.ptr;
    // fp16 boxes reach up to one half ulp (2^-11 relative) past the f32 root box
    P.bvh_rr_h = std::nextafter(B.root_radius * (1.0f + 0x1p-9f), INFINITY);
    P.bvh_nnodes = (uint32_t)B.nodes.size();
    // (the large list in LDS too: LLARGE_CAP; the leaf spheres: a leaf word in a 16-bit walk-stack entry)
    // (bvh_walk_noovf's paired leaf pass is written out for leaves of at most hrt_dev::BVH_MAX_LEAF spheres)
    static_assert(hrt::BVH_MAX_LEAF == hrt_dev::BVH_MAX_LEAF, "the builder's leaf size is the kernels'");
    P.bvh_lnodes = (B.nodes.size() <= hrt_dev::LNODE_CAP && B.depth <= hrt_dev::LNODE_DEPTH &&
                    B.large.size() <= hrt_dev::LLARGE_CAP && B.slot.size() <= hrt_dev::LNODE_LEAF_SPHERES) ? 1u : 0u;
    // (0 auto = off: the packet walk measured -8 % on C3)
    P.packet = (P.bvh_lnodes && r->params.packet == 2u) ? 1u : 0u;
    // delta = 8u r_max + min(16u D^2 / r_min, 2e-3 D) + 4u D + 4e-23/|d|  (u = 2^-24)
    const float u = 0x1p-24f;
    P.pad_k1 = 8.0f * u * B.r_max;
    P.pad_k2 = B.r_min > 0.0f ? 16.0f * u / B.r_min : INFINITY;
    P.pad_k3 = 2e-3f;
    P.pad_k4 = 4.0f * u;
    P.bq_nlarge = P.nlarge;
    for (int k = 0; k < 3; k++) P.bq_rc[k] = P.bvh_rc[k];
    P.bq_rr_h = P.bvh_rr_h;
    P.bq_k1 = P.pad_k1;
    P.bq_k2 = P.pad_k2;
    P.bq_k3 = P.pad_k3;
    P.bq_k4 = P.pad_k4;
    // code_aux's records: the BVH codes, the large list, then every slot (upload_spheres bounds the size)
    P.code_aux_bytes = r->code_aux.ptr == nullptr
                           ? 0u
                           : (uint32_t)((B.slot.size() + B.large.size() + (size_t)r->n_spheres) * sizeof(hrt_dev::SphereAux));
    return RT_OK;
}

// What the tile lists are a function of, besides the leaf spheres (rt_tile_lists.hpp): the camera constants and row share
// of scene_params, 8x8 tiles over W x nrows, and K.
hrt_tiles::View tile_view_of(const hrt_dev::KParams& P, uint32_t k_list) {
    hrt_tiles::View V;
    std::memset(&V, 0, sizeof V);  // (the padding too: views are compared as bytes)
    for (int i = 0; i < 4; i++) {
        V.eye[i] = P.cam.eye[i];
        V.dir[i] = P.cam.dir[i];
        V.up[i] = P.cam.up[i];
        V.right[i] = P.cam.right[i];
    }
    V.focal = P.cam.focal;
    V.blur = P.cam.blur;
    V.k = P.cam.k;
    V.aspect = P.cam.aspect;
    V.wm1 = P.cam.wm1;
    V.hm1 = P.cam.hm1;
    V.W = P.W;
    V.H = P.H;
    V.row0 = P.row0;
    V.row_block = P.row_block;
    V.row_stride = P.row_stride;
    V.nrows = P.nrows;
    V.tiles_w = (P.W + 7u) / 8u;
    V.tiles_h = (P.nrows + 7u) / 8u;
    V.k_list = std::min(k_list, hrt_tiles::K_MAX);
    return V;
}

// The lists for P's view, built on the device unless the renderer holds them already. A camera that moves rebuilds them
// every draw: one thread per tile over the leaf spheres, no scratch (C3: 32,400 tiles x 483 spheres).
int ensure_tile_lists(rt_renderer* r, const hrt_dev::KParams& P) {
    const hrt_tiles::View V = tile_view_of(P, r->tile_list_k);
    if (r->tile_lists_valid && std::memcmp(&V, &r->tile_view, sizeof V) == 0) return RT_OK;
    r->tile_lists_valid = false;
    const size_t ntiles = (size_t)V.tiles_w * V.tiles_h;
    int rc = ensure(r->tile_lists, std::max<size_t>(ntiles * hrt_tiles::WORDS, 1));
    if (rc) return rc;
    HIP_TRY(hrt_launch_tile_lists(V, r->bvh_sph.ptr, P.bvh_nleaf, r->tile_lists.ptr, r->stream));
    r->tile_view = V;
    r->tile_lists_valid = true;
    return RT_OK;
}

// k_trace_split<LNODES, false, false, false> answers a listed tile's primary rays when it makes their frame block
// (rt_kernels.hip trace_split, BLOCKRES): the sphere program's culling walk with the nodes in LDS, the sample buffer, no
// counting, no packets, a bounce cap of at least 1 (a launch that steals runs another kernel: launch_frames).
bool tile_lists_wanted(const rt_renderer* r, const hrt_dev::KParams& P, int variant) {
    return r->tile_list_mode != 1u && r->mode == RT_MODE_SPHERE && variant == hrt_dev::SCAN_BVH && P.bvh_lnodes && !P.packet &&
           !P.count_tests && P.bounces >= 1u && P.bvh_nleaf > 0u &&
           (uint64_t)P.bvh_nleaf + P.nlarge < hrt_dev::TILE_LIST_CODES;
}

int launch_frames(rt_renderer* r, uint32_t count, uint32_t time0, uint32_t dtime) {
    if (!r->has_camera) return fail(RT_ERR_STATE, "rt_set_camera must be called before drawing");
    hrt_dev::KParams P{};
    int rc = scene_params(r, P);
    if (rc) return rc;
    // RT_RAW_COUNTERS exported words, then the sample queue's fold-ring watchdog (rt_kernels.hip idle_spin)
    rc = ensure(r->counter, hrt_dev::COUNTER_WORDS);
    if (!rc) rc = ensure(r->count_spread, (size_t)hrt_dev::CSPREAD * hrt_dev::CSTRIDE);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(r->counter.ptr, 0, hrt_dev::COUNTER_WORDS * sizeof(unsigned long long), r->stream));
    HIP_TRY(hipMemsetAsync(r->count_spread.ptr, 0, (size_t)hrt_dev::CSPREAD * hrt_dev::CSTRIDE * sizeof(unsigned long long),
                           r->stream));
    P.dtime = dtime;
    P.bounces = r->params.bounces;
    P.ema_cap = (float)r->params.ema_cap;
    P.image = r->image.ptr;
    P.count_tests = r->params.count_tests;
    P.counter = r->counter.ptr;
    P.count_spread = r->count_spread.ptr;
#ifdef HRT_STAMPS
    {
        // k_render's waves, or the persistent kernels' (at most steal_cap = 32 per CU)
        const size_t wave_words = 8ull * std::max<size_t>((size_t)((r->width + 15u) / 16u) * ((P.nrows + 15u) / 16u) * 4u,
                                                          32ull * std::max(r->cus, 1u));
        const size_t words = wave_words + (1ull << 21);  // + one word per job (k_trace's job_trace)
        int rc2 = ensure(r->wave_trace, words);
        if (rc2) return rc2;
        HIP_TRY(hipMemsetAsync(r->wave_trace.ptr, 0, words * sizeof(unsigned long long), r->stream));
        r->wave_trace_words = words;
        P.wave_trace = r->wave_trace.ptr;
        P.job_trace = r->wave_trace.ptr + wave_words;
    }
#endif
    const int variant = r->mode == RT_MODE_TRIS ? hrt_dev::SCAN_SIMPLE : resolve_variant(r);
    const uint32_t schedule = resolve_schedule(r, count);
    r->last_variant = variant;
    r->last_schedule = schedule;
    r->last_suspend = 0;

    uint32_t launches = 0, ordered = 0;
    hrt_reset_last_kernel();  // (a draw that launches nothing reports no kernel)
    if (P.nrows == 0u) {  // a renderer that owns no rows (row0 at or below the last row): nothing to trace
        r->trace_pairs = 0;
        HIP_TRY(hipEventRecord(r->ev_start, r->stream));
    } else if (schedule == RT_SCHEDULE_QUEUE) {
        r->trace_pairs_pending = 0;
        P.tiles_w = (r->width + 7u) / 8u;
        P.tiles_h = (P.nrows + 7u) / 8u;
        const uint32_t ntiles = P.tiles_w * P.tiles_h;
        // suspendable walks (k_trace_split / k_trace_split_tris): the sphere program's culling BVH, the heap walk
        // of the triangle / mixed programs; not the opt-in SAH walk
        const bool split = !P.tri_bvh && (r->mode != RT_MODE_SPHERE || variant == hrt_dev::SCAN_BVH);
        // k_trace_split_tris<.., HL > 0> (heap top in LDS, 8 leaf-pair list words per lane): the mixed program's
        // sphere walk (culling BVH, begin phase) fits an 8-entry stack (a path holds at most depth pending siblings;
        // deeper trees would only fall back to the exact full scan, but keep the 16-entry kernel for them)
        // (and heaps of at most 2^24 nodes: node_hit_so addresses node i with a 24-bit multiply-add)
        P.tri_small = 0u;
        if (r->mode != RT_MODE_SPHERE &&
            (r->mode == RT_MODE_TRIS || variant != hrt_dev::SCAN_BVH || r->bvh_host.depth <= 8u) && r->params.heap_lds != 1u &&
            r->bvh_n <= (1u << 24))
            P.tri_small = HEAP_AUTO;
        if (variant == hrt_dev::SCAN_DEFER && r->mode == RT_MODE_MIXED && P.tri_small > 1u) P.tri_small = 1u;
        // job_frames 0 = per kernel: 32 for the suspendable walks (C3 +0.7 %, C4 +1.5 % over 16), 16 for k_trace's
        // cheap sphere scans (C2: 32 costs 3 %); a power of two (the ring's slot layout)
        uint32_t jf = r->params.job_frames ? r->params.job_frames : (split ? 32u : 16u);
        P.jf_log2 = 0;
        while ((2u << P.jf_log2) <= std::min(jf, 1024u)) P.jf_log2++;
        jf = 1u << P.jf_log2;
        // How the colours are folded (rt_params.queue_budget_mb, fold): the sample buffer (every colour
        // of a launch, then k_accumulate) in launches of equal frame counts, or the bounded-memory fold ring.
        //   queue_budget_mb 0 (auto, the default): floor(count / 320) launches (at least one) of whole jobs. A launch of
        //     320+ frames loses ~2 % to one launch of every frame (C3 3 x 342 frames: 33.8 vs 34.5 Grays/s), shorter ones
        //     lose more (fewer jobs per tile spread the waves over more of the image; C3 at 82 / 164 frames 29.3 / 31.5,
        //     C4 in launches of 345 + 167 frames -13 %), so the buffer holds at most ~640 frames (C3: 8.8 GB, not 25.5),
        //     or every frame that fits AUTO_FIT if that is more, and at most AUTO_BUDGET;
        //   queue_budget_mb > 0: a cap in MiB, launches of as many frames as it holds, balanced;
        //   the fold ring (fold 0) when a launch would get fewer than min(count, 320) frames.
        // (Pipelined launches of tile-row bands x every frame, which keep every frame of a tile in one launch within a
        // bounded buffer, measured bit-identical but slower than these launches at the same budget: C3 tie, C4 -13 %,
        // C5 -19 %; profiles/r04/band/.)
        constexpr size_t AUTO_BUDGET = 32768ull << 20, AUTO_FIT = 8192ull << 20;
        const size_t frame_floats = (size_t)ntiles * 64u * 3u;  // tile-padded
        const size_t frame_bytes = frame_floats * 4u;
        const uint32_t nframes_all = std::max(count, 1u);
        size_t budget = (size_t)r->params.queue_budget_mb << 20;
        // equal launches of at most `fit` frames, rounded up to whole jobs where that still fits: every launch but the
        // last then holds whole jobs, so the tail split applies (C3: 352 + 352 + 320 frames, not 3 x 342)
        auto balanced = [&](size_t fit) {
            fit = std::max<size_t>(1, std::min<size_t>(fit, nframes_all));
            const size_t n = (nframes_all + fit - 1u) / fit;
            const size_t c = (nframes_all + n - 1u) / n, cj = (c + jf - 1u) / jf * jf;
            return (uint32_t)(cj <= fit ? cj : c);
        };
        if (r->params.queue_budget_mb == 0u) {
            // the 320-frame rule, or as many frames as AUTO_FIT holds when that is more (a renderer with few rows —
            // a rank of a multi-GPU render, C3 / 8 = 3.2 GB — draws in one launch, without the extra drains)
            const uint32_t n = std::max(1u, nframes_all / 320u);
            const size_t c = (nframes_all + n - 1u) / n, cj = (c + jf - 1u) / jf * jf;
            const size_t frames =
                std::max(std::min<size_t>(cj, nframes_all), std::min<size_t>(AUTO_FIT / frame_bytes, nframes_all));
            budget = std::min(AUTO_BUDGET, frames * frame_bytes);
        }
        uint32_t chunk = balanced(budget / frame_bytes), log2s = 0;
        P.ring_mode = chunk < std::min(nframes_all, 320u) ? 1u : 0u;
        if (r->params.fold == RT_FOLD_BUFFER || r->params.fold == RT_FOLD_NEXT) P.ring_mode = 0u;  // forced (measurements, tests)
        if (r->params.fold == RT_FOLD_RING) P.ring_mode = 1u;
        const size_t fail_above = (size_t)r->test_fail_alloc_above_mb << 20;
        size_t zero_words = 0;
        if (!P.ring_mode) {
            r->ring.release();  // the other fold's memory: the draw's colour memory stays within the budget
            r->ring_ctl.release();
            // k_trace_split carries a sample's index in the launch's buffer in 32 bits (KParams::sample_npix): a launch holds
            // fewer than 2^32 samples (48 GiB of colours; the automatic budget stays below it)
            const uint64_t idx_fit = 0xFFFFFFFFull / ((uint64_t)ntiles * 64u);
            if (chunk > idx_fit) chunk = balanced((size_t)idx_fit);
            // a device short of memory gets smaller launches, down to one frame, instead of a failed draw
            const size_t buf_budget = std::max(budget, frame_bytes);
            while ((rc = ensure_within(r->samples, (size_t)chunk * frame_floats, buf_budget, fail_above)) == RT_ERR_ALLOC &&
                   chunk > 1u) {
                (void)hipGetLastError();  // clear the failed hipMalloc's sticky status
                chunk = (chunk + 1u) / 2u;
            }
            if (rc) return rc;
            P.samples = r->samples.ptr;
            r->ring_slots = 0;
            r->fold_bytes = (uint64_t)chunk * frame_bytes;
        } else {
            r->samples.release();
            // frames per launch: at most FOLD_MAX_JOBS jobs per tile (the done bits of the tile's fold word)
            chunk = std::max(1u, std::min(count, hrt_dev::FOLD_MAX_JOBS * jf));
            const uint32_t nchunks_max = (chunk + jf - 1u) / jf;
            // a power-of-two number of job slots (jf x 64 px x 16 B each) in the budget, at most one per job of a
            // launch; a device short of memory gets a halved budget instead of a failed draw
            budget = std::min<size_t>(budget, 2047ull << 20);
            const uint64_t jobs = (uint64_t)ntiles * nchunks_max;
            for (;;) {
                const size_t fit = std::max<size_t>(1, budget / ((size_t)jf << 10));
                log2s = 0;
                while ((2ull << log2s) <= fit && (1ull << log2s) < jobs && log2s < 20u) log2s++;
                // rt_testing_set_faults caps the slots (tests: jobs then wait in the free queue for a slot)
                while (r->test_ring_slots_max && log2s > 0 && (1ull << log2s) > r->test_ring_slots_max) log2s--;
                zero_words = 2ull * ntiles + (4ull << log2s) + 4u;
                const size_t ring_floats4 = ((size_t)jf << log2s) * 64u;
                rc = ensure_within(r->ring, ring_floats4, std::max(budget, ring_floats4 * 16u), fail_above);
                const size_t ctl_words = zero_words + (size_t)ntiles * nchunks_max;
                if (!rc) rc = ensure_within(r->ring_ctl, ctl_words, ctl_words * 4u, fail_above);
                if (rc != RT_ERR_ALLOC || budget <= ((size_t)jf << 10)) break;
                (void)hipGetLastError();
                r->ring.release();  // retry both with half the budget
                r->ring_ctl.release();
                budget /= 2u;
            }
            if (rc) return rc;
            P.ring = r->ring.ptr;
            P.ring_log2 = log2s;
            P.ring_bytes = (uint32_t)(((size_t)jf << log2s) * 1024u);
            P.tile_fold = (unsigned long long*)r->ring_ctl.ptr;
            P.ring_q = r->ring_ctl.ptr + 2ull * ntiles;
            P.ring_tail = P.ring_q + (4u << log2s);
            P.job_slot = r->ring_ctl.ptr + zero_words;
            r->ring_slots = 1u << log2s;
            r->ring_tiles = ntiles;
            r->ring_ctl_words = zero_words + (size_t)ntiles * nchunks_max;
            r->fold_bytes = (uint64_t)P.ring_bytes + 4ull * (4u * r->ring_slots + 4u) + 4ull * r->ring_ctl_words -
                            4ull * zero_words + 8ull * ntiles;
        }
        // frame-block work stealing (rt_kernels.hip steal_block): the suspendable-walk kernels with the sample
        // buffer; one slot per resident wave, at most 32 waves per CU
        P.steal_cap = 32u * std::max(r->cus, 1u);
        rc = ensure(r->steal_slots, P.steal_cap);
        if (rc) return rc;
        P.steal_slots = r->steal_slots.ptr;
        // Cost-ordered dealing (rt_params.cost_order; rt_kernels.hip k_order_*): a learning launch counts its samples'
        // queries per pixel and the tiles are split into the most expensive half, sorted by cost, and the rest in
        // raster order; the following launches (of this draw and the next ones) deal that head first, so the jobs that
        // take longest start early instead of trailing the launch. The renderer learns in its first ordered launch after
        // any scene, camera, size, row, bounce-cap, slot or triangle-walk change (cost_order 3: in every launch).
        // Auto: a rank's share of a row partition (row_step > 1), which then does not steal, and the suspendable-walk
        // kernels' full images — measured (profiles/r05/t/, u/, y/): 8-way splits C3 0.940 -> 0.96, C5 0.974 -> 0.987,
        // C2 0.52 -> 0.66 and C4 0.755 -> 0.84 with the short-launch job size below; full images C3 +0.6 %, C5 +0.3 %,
        // C4 flat, C2 (k_trace, not ordered) -1.5 %. Bit-identical in any order.
        const bool order_any = !P.ring_mode && r->params.cost_order != 1u;
        // (full images too for the suspendable-walk kernels: C3 38.29 -> 38.53 Grays/s, C5 +0.3 %, C4 flat; not for
        // k_trace's full images: C2 -1.5 %; profiles/r05/y/)
        const bool want_order = order_any && (r->params.cost_order >= 2u || r->params.row_step > 1u || split);
        // Short launches (a rank's share of a row partition, small images): fewer than 32 jobs per resident wave at the
        // kernel's job size. Their jobs are halved (job_frames 0 only), so a job on a costly tile no longer outlasts the
        // launch: C4's 8-way shares in cost order 0.43 with 32-frame jobs, 0.82 with 16; C2's shares 1.00 ms with 8-frame
        // jobs against 1.16 with 16, C3's flat (profiles/r05/r/, t/). Long launches keep the larger jobs (C2 full image
        // -2.6 % with 8, C4 -1.2 % with 16).
        if (!P.ring_mode && r->params.job_frames == 0u && jf > 1u &&
            (uint64_t)ntiles * ((chunk + jf - 1u) / jf) < 32ull * 24u * std::max(r->cus, 1u)) {
            jf >>= 1;
            P.jf_log2--;
        }
        P.queue = r->counter.ptr + 15u;
        // the sample buffer's jobs from one counter per XCD
        constexpr size_t QWORDS = (size_t)hrt_dev::NQ * hrt_dev::QSTRIDE;
        P.queues = nullptr;
        if (!P.ring_mode) {  // (+ the fold counter, below)
            rc = ensure(r->queues, QWORDS + hrt_dev::QSTRIDE);
            if (rc) return rc;
        }
        // Each launch folds the one before (rt_params.fold 3; rt_kernels.hip fold_prev_tiles): two sample buffers, launch
        // k writes buffer k % 2 while every FOLD_WAVE_MOD-th wave first folds buffer (k - 1) % 2 into the image;
        // k_accumulate folds the last launch only. The suspendable-walk kernels, draws of two or more launches; auto with
        // the automatic colour budget (it doubles the colour memory: C3 17.5 GB). C3 38.38 -> 38.76-38.83 Grays/s with 1 in
        // 32 / 64 / 128 waves folding, 38.62-38.65 with 1 in 16, 38.30-38.44 with 1 in 1 or 4; C5 +0.2 %
        // (profiles/r06/fold_next/).
        constexpr uint32_t FOLD_WAVE_MOD = 64;
        bool fold_next = !P.ring_mode && split && count > chunk &&
                         (r->params.fold == RT_FOLD_NEXT || (r->params.fold == RT_FOLD_AUTO && r->params.queue_budget_mb == 0u));
        if (fold_next) {
            rc = ensure_within(r->samples2, (size_t)chunk * frame_floats, std::max(budget, frame_bytes), fail_above);
            if (rc == RT_ERR_ALLOC) {
                (void)hipGetLastError();
                fold_next = false;
            } else if (rc) {
                return rc;
            }
        }
        if (!fold_next) r->samples2.release();
        else r->fold_bytes *= 2u;
        r->last_fold_next = fold_next;
        // (suspend_below 0: the same kernels with a threshold no wave reaches, 1 walking lane: no suspension)
        P.suspend_below = split ? std::max(r->params.suspend_below, 1u) : 0u;
        // (the sphere program's split kernel takes its descent hold in the same word, bits 8..15)
        if (split && r->mode == RT_MODE_SPHERE) P.suspend_below |= r->descent_hold << 8;
        r->last_suspend = split ? r->params.suspend_below : 0u;
        P.job_frames = jf;
        HIP_TRY(hipEventRecord(r->ev_start, r->stream));
        const bool lists = split && !P.ring_mode && tile_lists_wanted(r, P, variant);
        P.fold_prev = nullptr;
        for (uint32_t done = 0, k = 0; done < count; done += chunk, k++) {
            if (fold_next) {
                P.samples = (k & 1u) ? r->samples2.ptr : r->samples.ptr;
                if (k > 0u) {  // the launch before: its buffer, frames and first frame
                    P.fold_prev = (k & 1u) ? r->samples.ptr : r->samples2.ptr;
                    P.fold_nframes = P.nframes;
                    P.fold_frame0 = P.frame0;
                    P.fold_next = (uint32_t*)(r->queues.ptr + QWORDS);
                    P.fold_mod = FOLD_WAVE_MOD;
                    HIP_TRY(hipMemsetAsync(P.fold_next, 0, sizeof(uint32_t), r->stream));
                }
            }
            P.nframes = std::min(chunk, count - done);
            P.time0 = time0 + done * dtime;
            P.frame0 = r->frame_count + done;
            P.nchunks = (P.nframes + P.job_frames - 1u) / P.job_frames;
            P.njobs = (unsigned long long)ntiles * P.nchunks;
            // Auto stealing: on for launches with fewer than 16 jobs per resident wave (about 24 per CU), where a job
            // dealt late can outlast the launch (C4's 8-way split: 0.47 -> 0.71 of the full image's rate); off for
            // long launches, where the claims cost 2-4 % and there is no tail to win back (C3: 8-way split 0.90 ->
            // 0.88)
            {
                const bool fits = ntiles < (1u << 25) - 1u && P.nchunks < 2048u;  // the slot's tile and chunk fields
                // (not once the launch can deal in cost order: C4's 8-way shares 0.755 with stealing, 0.82 in order)
                const bool want = r->params.steal == 2u ||
                                  (r->params.steal == 0u && P.njobs < 16ull * 24u * std::max(r->cus, 1u) &&
                                   !(want_order && r->order_tiles == ntiles));
                // (k_trace's frame-block refill for the linear sphere scan with the same stealing ran 3x slower, C2 80 ->
                // 26 Grays/s: a claim per 64 cheap samples stalls the wave; profiles/r05/o/)
                P.steal = (split && !P.ring_mode && fits && want) ? 1u : 0u;
            }
            // The tile lists, built by the first launch that reads them: a launch that steals runs another kernel, so a
            // draw of short launches (a rank's share) never pays for lists. Inside the draw's timing, outside the launch's
            // own pair of events: the first draw of a view shows their cost in its rt_stats, later draws find them built —
            // bench.py's warmup pays for them, not every step.
            P.tile_lists = nullptr;
            if (lists && !P.steal) {
                rc = ensure_tile_lists(r, P);
                if (rc) return rc;
                P.tile_lists = r->tile_lists.ptr;
            }
            // Tail split (the suspendable-walk kernels with the sample buffer, no stealing): the last ~2 jobs per
            // resident wave are dealt in parts (rt_params.tail_split: 2 quarters, 3 eighths; 0 auto = quarters),
            // so the launch's drain waits for a part, not a whole job (job_frames a multiple of the part count and
            // whole chunks only; tail_split 1 turns it off)
            P.tail_from = 0xFFFFFFFFu;
            P.tail_shift = r->params.tail_split == 3u ? 3u : 2u;
            // (k_trace's frame-block refill could decode them too, without spills: C2's full image ran 9 % slower with the
            // parts, 74.1 vs 81.3 Grays/s, for its 8-way split 0.51 -> 0.55; round 5, profiles/r05/f/)
            if (split && P.suspend_below > 0u && !P.ring_mode && !P.steal && P.job_frames % (1u << P.tail_shift) == 0u &&
                P.nframes % P.job_frames == 0u && r->params.tail_split != 1u && P.njobs < (1ull << 29)) {
                const unsigned long long q = std::min<unsigned long long>(P.njobs, 64ull * std::max(r->cus, 1u));
                P.tail_from = (uint32_t)(P.njobs - q);
                P.njobs += ((1ull << P.tail_shift) - 1u) * q;
            }
            r->ring_nchunks = P.nchunks;
            HIP_TRY(hipMemsetAsync(P.queue, 0, sizeof(unsigned long long), r->stream));
            // (not with stealing: its launches are short, and the per-XCD fetch spilled SGPRs in the stealing kernels)
            P.queues = !P.ring_mode && !P.steal ? r->queues.ptr : nullptr;
            if (P.queues) HIP_TRY(hipMemsetAsync(P.queues, 0, QWORDS * sizeof(unsigned long long), r->stream));
            if (P.steal) HIP_TRY(hipMemsetAsync(P.steal_slots, 0, P.steal_cap * sizeof(unsigned long long), r->stream));
            if (P.ring_mode) HIP_TRY(hipMemsetAsync(r->ring_ctl.ptr, 0, zero_words * sizeof(uint32_t), r->stream));
            rc = trace_events(r, r->trace_pairs_pending);
            if (rc) return rc;
            HIP_TRY(hipEventRecord(r->ev_trace[2 * r->trace_pairs_pending], r->stream));
            const bool order_on = want_order && (r->params.cost_order >= 2u || !P.steal);
            if (want_order && r->cost_tiles != ntiles) {
                const size_t SCRATCH = hrt_order_scratch_words(ntiles);
                rc = ensure(r->tile_cost, (size_t)ntiles * 64u);
                if (!rc) rc = ensure(r->tile_sum, ntiles);
                if (!rc) rc = ensure(r->tile_order, ntiles);
                if (!rc) rc = ensure(r->order_scratch, SCRATCH);
                if (rc) return rc;
                HIP_TRY(hipMemsetAsync(r->tile_cost.ptr, 0, (size_t)ntiles * 64u * sizeof(uint32_t), r->stream));
                HIP_TRY(hipMemsetAsync(r->order_scratch.ptr, 0, SCRATCH * sizeof(uint32_t), r->stream));
                r->cost_tiles = ntiles;
                r->order_tiles = 0;
                r->cost_learn = true;
            }
            P.tile_order = order_on && r->order_tiles == ntiles ? r->tile_order.ptr : nullptr;
            ordered += P.tile_order ? 1u : 0u;
            // (a launch that steals still learns, so the next one can deal in cost order instead)
            const bool learn = want_order && (r->cost_learn || r->params.cost_order == 3u);
            P.tile_cost = learn ? r->tile_cost.ptr : nullptr;
            P.sample_npix = ntiles * 64u;
            if (!P.ring_mode && (uint64_t)P.nframes * P.sample_npix > 0xFFFFFFFFull)  // (the launch's sizing above)
                return fail(RT_ERR_STATE, "a sample-buffer launch of 2^32 samples or more");
            HIP_TRY(hrt_launch_trace(r->mode, variant, P, r->stream));
            HIP_TRY(hipEventRecord(r->ev_trace[2 * r->trace_pairs_pending + 1], r->stream));
            r->trace_pairs_pending++;
            launches++;
            if (learn) {  // (three small kernels, not counted in rt_stats.launches)
                HIP_TRY(hrt_launch_order(r->tile_cost.ptr, ntiles, r->tile_sum.ptr, r->tile_order.ptr, r->order_scratch.ptr,
                                         r->stream));
                r->order_tiles = ntiles;
                r->cost_learn = false;
            }
            if (!P.ring_mode && (!fold_next || done + chunk >= count)) {
                HIP_TRY(hrt_launch_accumulate(P, r->stream));
                launches++;
            }
        }
        r->last_launch_frames = chunk;
        r->last_ordered = ordered;
        r->trace_pairs = r->trace_pairs_pending;
        r->trace_pairs_pending = 0;
    } else {
        const uint32_t fpl = std::max<uint32_t>(1u, r->params.frames_per_launch);
        HIP_TRY(hipEventRecord(r->ev_start, r->stream));
        for (uint32_t done = 0; done < count; done += fpl) {
            P.nframes = std::min(fpl, count - done);
            P.time0 = time0 + done * dtime;
            P.frame0 = r->frame_count + done;
            HIP_TRY(hrt_launch_render(r->mode, variant, P, r->stream));
            launches++;
        }
        r->trace_pairs = 0;  // k_render is the whole draw: trace time = kernel time
    }
    HIP_TRY(hipEventRecord(r->ev_stop, r->stream));
    r->frame_count += count;  // end_frame, renderer.rs:409
    r->stats = rt_stats{};
    r->stats.samples = (uint64_t)count * P.nrows * r->width;
    r->stats.launches = launches;
    r->stats.local_rows = P.nrows;
    std::snprintf(r->stats.kernel, sizeof r->stats.kernel, "%s", hrt_last_kernel());
    if (schedule == RT_SCHEDULE_QUEUE && count && P.nrows) {
        r->stats.fold_ring = P.ring_mode ? 1u : r->last_fold_next ? 2u : 0u;
        r->stats.fold_bytes = r->fold_bytes;
        r->stats.launch_frames = std::min(count, r->last_launch_frames);
        r->stats.ordered_launches = r->last_ordered;
    }
    r->stats.device_bytes = r->device_bytes();
    r->timing_pending = true;
    return RT_OK;
}

int finish_stats(rt_renderer* r) {
    if (!r->timing_pending) return RT_OK;
    HIP_TRY(hipEventSynchronize(r->ev_stop));
    float ms = 0.0f;
    HIP_TRY(hipEventElapsedTime(&ms, r->ev_start, r->ev_stop));
    unsigned long long* q = r->raw_counters;
    unsigned long long wd[4] = {};
    HIP_TRY(hipMemcpy(q, r->counter.ptr, RT_RAW_COUNTERS * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    {  // the work counters' copies (rt_kernels.hip flush_counts) into words 0-4
        std::vector<unsigned long long> sp((size_t)hrt_dev::CSPREAD * hrt_dev::CSTRIDE);
        HIP_TRY(hipMemcpy(sp.data(), r->count_spread.ptr, sp.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (uint32_t k = 0; k < hrt_dev::CSPREAD; k++)
            for (uint32_t c = 0; c < 5u; c++) q[c] += sp[(size_t)k * hrt_dev::CSTRIDE + c];
        r->blocks_resolved = 0;  // (word 5: the frame blocks resolved when made, rt_testing_get_tile_lists_resolved)
        for (uint32_t k = 0; k < hrt_dev::CSPREAD; k++) r->blocks_resolved += sp[(size_t)k * hrt_dev::CSTRIDE + 5u];
    }
    HIP_TRY(hipMemcpy(wd, r->counter.ptr + hrt_dev::WATCHDOG, sizeof wd, hipMemcpyDeviceToHost));
    if (wd[0] || wd[3]) {  // waves gave up waiting for a fold-ring slot: the image is incomplete; report, do not hang
        // diagnostic build: HRT_RING_DUMP=path writes the fold-ring control words (tile done masks, tile locks and
        // cursors, free queue, tail) and the counters as raw little-endian words
#ifdef HRT_STAMPS
        if (const char* path = std::getenv("HRT_RING_DUMP")) {
            std::vector<uint32_t> ctl(r->ring_ctl_words);
            if (!ctl.empty())
                HIP_TRY(hipMemcpy(ctl.data(), r->ring_ctl.ptr, ctl.size() * 4u, hipMemcpyDeviceToHost));
            unsigned long long cnt[hrt_dev::COUNTER_WORDS];
            HIP_TRY(hipMemcpy(cnt, r->counter.ptr, sizeof cnt, hipMemcpyDeviceToHost));
            if (FILE* f = std::fopen(path, "wb")) {
                const uint32_t hdr[4] = {r->ring_tiles, r->ring_slots, r->ring_nchunks, (uint32_t)ctl.size()};
                std::fwrite(hdr, 4, 4, f);
                std::fwrite(cnt, 8, hrt_dev::COUNTER_WORDS, f);
                std::fwrite(ctl.data(), 4, ctl.size(), f);
                std::fclose(f);
            }
        }
#endif
        char msg[200];
        std::snprintf(msg, sizeof msg, "sample queue: %llu waves waited > 2^24 idle rounds for a fold-ring slot "
                      "(last: job %llu, entry flags %llx); %llu free-queue overruns", wd[0], wd[1], wd[2], wd[3]);
        r->timing_pending = false;
        return fail(RT_ERR_DEVICE, msg);
    }
    r->stats.kernel_ms = ms;
    r->stats.trace_ms = ms;
    r->stats.trace_launches = r->stats.launches;
    if (r->trace_pairs) {
        double tms = 0.0;
        for (uint32_t k = 0; k < r->trace_pairs; k++) {
            float e = 0.0f;
            HIP_TRY(hipEventElapsedTime(&e, r->ev_trace[2 * k], r->ev_trace[2 * k + 1]));
            tms += e;
        }
        r->stats.trace_ms = tms;
        r->stats.trace_launches = r->trace_pairs;
    }
    r->stats.queries = q[0];
    r->stats.box_tests = q[1];
    r->stats.sphere_tests = q[2];
    r->stats.node_tests = q[3];
    r->stats.tri_tests = q[4];
    r->stats.variant = (uint32_t)r->last_variant;
    r->stats.schedule = r->last_schedule;
    r->stats.suspend_below = r->last_suspend;
    r->timing_pending = false;
    return RT_OK;
}

void delete_buffers(rt_renderer* r) {
    r->image.release();
    r->sph_geo.release();
    r->sph_aux.release();
    r->code_aux.release();
    r->sph_pairs.release();
    r->bvh_nodes.release();
    r->bvh_sph.release();
    r->bvh_hnodes.release();
    r->bvh_slot.release();
    r->bvh_large.release();
    r->nodes.release();
    r->nodes_so.release();
    r->tris.release();
    r->tri_geo.release();
    r->mats.release();
    r->tb_hnodes.release();
    r->tb_order.release();
    r->tb_parent.release();
    if (r->refit_stat_host) (void)hipHostFree(r->refit_stat_host);
    r->refit_stat_host = nullptr;
    r->lb_tris.release();
    r->lb_geo.release();
    r->lb_mats.release();
    r->lb_hnodes.release();
    r->lb_order.release();
    r->lb_keys.release();
    r->lb_parent.release();
    r->lb_arrivals.release();
    r->lb_boxes.release();
    r->lb_stat.release();
    r->counter.release();
    r->count_spread.release();
    r->steal_slots.release();
    r->queues.release();
    r->samples.release();
    r->samples2.release();
    r->ring.release();
    r->ring_ctl.release();
    r->wave_trace.release();
    r->tile_cost.release();
    r->tile_sum.release();
    r->tile_order.release();
    r->tile_lists.release();
    for (CounterSlot* c : {&r->closest_count, &r->winding_count, &r->multihit_count, &r->overlap_count}) c->buf.release();
    r->tb_moments.release();
    r->moments_dirty = true;
    r->tile_lists_valid = false;
    r->order_scratch.release();
    r->cost_tiles = r->order_tiles = 0;
}

// True when one of `ptrs` is not a multiple of `align` bytes. Null passes: an optional buffer that was not given.
bool misaligned(size_t align, std::initializer_list<const void*> ptrs) {
    for (const void* p : ptrs)
        if ((uintptr_t)p % align) return true;
    return false;
}

// The refusals of a call that reads the triangle tree. any_tree: a tree the call itself has built when there is none (the
// read-outs of the tree), so only the sphere program is refused.
int need_tri_tree(const rt_renderer* r, const char* who, bool any_tree = false) {
    if (r->mode == RT_MODE_SPHERE) return fail(RT_ERR_ARG, std::string(who) + ": the sphere program has no triangle tree");
    if (!any_tree && !r->dev_geom && !r->params.tri_bvh)
        return fail(RT_ERR_STATE, std::string(who) + ": no triangle tree (device geometry or rt_params.tri_bvh = 1 has one)");
    return RT_OK;
}

// What every ray query sets up once its arguments are checked, in this order: the renderer's device made current, the
// scene's kernel arguments (scene_params) and the scan variant a tiles draw would run. rc: the first failure. A query on
// the triangle tree names itself in tree_who: need_tri_tree's refusals come first then, and scene_params has uploaded the
// tree (upload_tri_tree builds a host SAH tree that is not built yet).
struct QueryScope {
    DeviceScope ds;
    hrt_dev::KParams P{};
    int variant = hrt_dev::SCAN_SIMPLE, rc;
    explicit QueryScope(rt_renderer* r, const char* tree_who = nullptr)
        : ds(r->device, tree_who ? need_tri_tree(r, tree_who) : RT_OK), rc(ds.rc) {
        if (!rc) rc = scene_params(r, P);
        if (!rc && r->mode != RT_MODE_TRIS) variant = resolve_variant(r);
    }
};

// The tree fields of a tree query's launch arguments (rt_closest.hpp Launch itself; the Tree of the other three), from the
// scene's kernel arguments.
template <typename T>
void tree_fields(T& t, const hrt_dev::KParams& P) {
    t.hnodes = (const hrt_lbvh::U4*)P.tb_hnodes;
    t.order = P.tb_order;
    t.geo = P.tri_geo;
    t.m = P.m;
    t.root = P.tb_root;
    for (int k = 0; k < 3; k++) t.rc[k] = P.tb_rc[k];
    t.rr_h = P.tb_rr_h;
}

}  // namespace

extern "C" {

const char* rt_last_error(void) { return g_last_error.c_str(); }

int rt_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* rt_build_info(void) {
    return "hrt gfx950 (HIP " HIP_VERSION_BUILD_NAME ") k_trace_split, k_trace_split_tris, k_trace, k_accumulate, "
           "k_render";
}

int rt_create(uint32_t width, uint32_t height, int mode, rt_renderer** out) {
    if (!out || width == 0 || height == 0) return fail(RT_ERR_ARG, "rt_create: null out or zero size");
    if (mode < RT_MODE_SPHERE || mode > RT_MODE_MIXED) return fail(RT_ERR_ARG, "rt_create: bad mode");
    *out = nullptr;
    int dev = 0;
    int rc = check_device(&dev);
    if (rc) return rc;
    rt_renderer* r = new rt_renderer();
    r->device = dev;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
            delete r;
            return fail(RT_ERR_DEVICE, "rt_create: hipDeviceGetAttribute(multiprocessor count) failed");
        }
        r->cus = (uint32_t)cus;
    }
    r->mode = mode;
    r->width = width;
    r->height = height;
    r->params.bounces = mode == RT_MODE_SPHERE ? 10u : 5u;  // BOUNCE_MAX
    r->params.ema_cap = RT_SAMPLE_FRAME;
    // arrayLength(&scene) = the 100-slot buffer in the sphere program; no such floor in the others.
    r->params.min_sphere_slots = mode == RT_MODE_SPHERE ? RT_MAX_OBJECT_IN_SCENE : 0u;
    r->params.row0 = 0;
    r->params.row_step = 1;
    r->params.row_block = 1;
    r->params.frames_per_launch = 32;
    r->params.schedule = RT_SCHEDULE_AUTO;
    // auto: balanced launches of 320-639 frames of whole jobs (C3: 352 + 352 + 320 frames, 8.8 GB of colours; launch_frames)
    r->params.queue_budget_mb = 0;
    // frames per 8x8-tile job; measured with the frame-block refill: C2 59.5 (8) -> 69.1 (16) -> 68.2 (32),
    // C3 +1 % at 16, C4 equal at 8/16 and -13 % at 32, C5 +0.7 % at 16
    r->params.job_frames = 0;  // per kernel (rt_draw_frames)
    // measured: C3 (sphere) 0 -> 21.2, 8 -> 23.4, 16 -> 23.8, 24 -> 23.7, 32 -> 22.7 Grays/s (first split
    //           kernel); with the frame-block refill and 16-frame jobs 16 -> 25.2, 24 -> 25.9, 32 -> 25.2;
    //           C4 (mixed) 0 -> 7.02, 8 -> 7.74, 16 -> 8.00, 24 -> 8.15, 32 -> 8.22, 48 -> 7.92; round 4 (final
    //           kernels, profiles/r04/so/sweep_sb_mixed.txt): C4 24 = 32 (13.22), C5 16/20/24/28/32 -> 10.26/10.27/
    //           10.30/10.28/10.24: the mixed program takes 24 too, the triangle program keeps 32
    r->params.suspend_below = mode == RT_MODE_TRIS ? 32u : 24u;
    bool ok = hipStreamCreateWithFlags(&r->stream, hipStreamNonBlocking) == hipSuccess &&
              hipEventCreate(&r->ev_start) == hipSuccess && hipEventCreate(&r->ev_stop) == hipSuccess;
    if (!ok) {
        rt_destroy(r);
        return fail(RT_ERR_DEVICE, "rt_create: stream/event creation failed");
    }
    rc = zero_image(r);
    if (rc) {
        rt_destroy(r);
        return rc;
    }
    *out = r;
    return RT_OK;
}

int rt_destroy(rt_renderer* r) {
    if (!r) return RT_OK;
    DeviceScope ds(r->device);  // (frees on the renderer's device even if switching failed)
    if (r->stream) (void)hipStreamSynchronize(r->stream);
    delete_buffers(r);
    for (hipEvent_t e : r->ev_trace) (void)hipEventDestroy(e);
    if (r->ev_start) (void)hipEventDestroy(r->ev_start);
    if (r->ev_stop) (void)hipEventDestroy(r->ev_stop);
    if (r->stream) (void)hipStreamDestroy(r->stream);
    delete r;
    return RT_OK;
}

int rt_abi_version(uint32_t* version, uint32_t* params_bytes, uint32_t* stats_bytes) {
    if (version) *version = RT_ABI_VERSION;
    if (params_bytes) *params_bytes = (uint32_t)sizeof(rt_params);
    if (stats_bytes) *stats_bytes = (uint32_t)sizeof(rt_stats);
    return RT_OK;
}

int rt_get_params(const rt_renderer* r, rt_params* out) {
    if (!r || !out) return fail(RT_ERR_ARG, "rt_get_params: null");
    *out = r->params;
    return RT_OK;
}

int rt_set_params(rt_renderer* r, const rt_params* p) {
    if (!r || !p) return fail(RT_ERR_ARG, "rt_set_params: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    // (row0 >= height: the renderer owns no rows, e.g. a rank beyond the image's last row block; its draws
    // render nothing and its image is empty)
    if (p->row_step == 0) return fail(RT_ERR_ARG, "rt_set_params: bad row partition (row_step 0)");
    if ((uint64_t)p->row_step * std::max(p->row_block, 1u) > (1ull << 30))
        return fail(RT_ERR_ARG, "rt_set_params: row_step x row_block too large");
    if (p->variant != 0 && p->variant != 1 && p->variant != 3 && p->variant != 4)
        return fail(RT_ERR_ARG, "rt_set_params: unknown variant (0 auto, 1 simple, 3 deferred, 4 culling BVH)");
    if (p->schedule > RT_SCHEDULE_QUEUE) return fail(RT_ERR_ARG, "rt_set_params: unknown schedule");
    if (p->tri_bvh > 1) return fail(RT_ERR_ARG, "rt_set_params: tri_bvh must be 0 or 1");
    if (p->suspend_below > 64) return fail(RT_ERR_ARG, "rt_set_params: suspend_below must be 0..64");
    if (p->fold > RT_FOLD_NEXT)
        return fail(RT_ERR_ARG, "rt_set_params: fold must be 0 auto, 1 buffer, 2 ring or 3 buffers folded by the next launch");
    if (p->heap_lds > 2) return fail(RT_ERR_ARG, "rt_set_params: heap_lds must be 0 auto, 1 off or 2 on");
    if (p->steal > 2) return fail(RT_ERR_ARG, "rt_set_params: steal must be 0 auto, 1 off or 2 on");
    if (p->tail_split > 3) return fail(RT_ERR_ARG, "rt_set_params: tail_split must be 0 auto, 1 off, 2 quarters or 3 eighths");
    if (p->count_tests > 1) return fail(RT_ERR_ARG, "rt_set_params: count_tests must be 0 or 1");
    if (p->packet > 2) return fail(RT_ERR_ARG, "rt_set_params: packet must be 0 auto, 1 off or 2 on");
    if (p->cost_order > 3)
        return fail(RT_ERR_ARG, "rt_set_params: cost_order must be 0 auto, 1 off, 2 on or 3 on, learning in every launch");
    const bool rows_changed = p->row0 != r->params.row0 || p->row_step != r->params.row_step ||
                              std::max(p->row_block, 1u) != r->row_block();
    const bool slots_changed = p->min_sphere_slots != r->params.min_sphere_slots;
    // the tiles' costs (queries per sample) change with the rows, the bounce cap and the scene's slots or triangle walk,
    // not with the kernels' knobs (count_tests, job size, ...: bench.py toggles count_tests around every warmup step)
    if (rows_changed || slots_changed || p->bounces != r->params.bounces || p->tri_bvh != r->params.tri_bvh)
        r->cost_learn = true;
    r->params = *p;
    if (rows_changed) {
        r->frame_count = 0;
        int rc = zero_image(r);
        if (rc) return rc;
    }
    if (slots_changed && r->sph_geo.ptr) return upload_spheres(r);
    return RT_OK;
}

int rt_set_camera(rt_renderer* r, const void* camera80) {
    if (!r || !camera80) return fail(RT_ERR_ARG, "rt_set_camera: null");
    std::memcpy(&r->camera, camera80, sizeof(hrt::Camera));
    r->has_camera = true;
    r->cost_learn = true;
    return RT_OK;
}

int rt_set_spheres(rt_renderer* r, const void* spheres48, uint32_t n) {
    if (!r || (n && !spheres48)) return fail(RT_ERR_ARG, "rt_set_spheres: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    // a hit carries its slot in 29 bits (rt_kernels.hip Hit::id)
    if (n >= (1u << 28)) return fail(RT_ERR_ARG, "rt_set_spheres: more than 2^28 spheres");
    r->spheres.resize(n);
    if (n) std::memcpy(r->spheres.data(), spheres48, (size_t)n * sizeof(hrt::Sphere));
    r->cost_learn = true;
    return upload_spheres(r);
}

int rt_set_bvh(rt_renderer* r, const uint32_t sizes[2], const void* nodes32, uint32_t n_nodes, const void* tris64,
               uint32_t n_tris, const void* mats32, uint32_t n_mats) {
    if (!r || !sizes) return fail(RT_ERR_ARG, "rt_set_bvh: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    const uint32_t n = sizes[0], m = sizes[1];
    if (int rc = rt_host_check_bvh_sizes(sizes, n_nodes, n_tris, n_mats)) return rc;
    if ((n && !nodes32) || (m && !tris64) || (n_mats && !mats32)) return fail(RT_ERR_ARG, "rt_set_bvh: null buffer");
    r->cost_learn = true;
    const hrt::Triangle* T = (const hrt::Triangle*)tris64;
    std::vector<hrt_dev::TriDev> td(m);
    for (uint32_t j = 0; j < m; j++) {
        const hrt::Triangle& t = T[j];
        if (t.material >= n_mats) return fail(RT_ERR_ARG, "rt_set_bvh: triangle material index out of range");
        hrt_dev::TriDev d;
        d.a = float4{t.a.x, t.a.y, t.a.z, 0.0f};
        d.e1 = float4{t.b.x - t.a.x, t.b.y - t.a.y, t.b.z - t.a.z, 0.0f};  // edge1 = b - a
        d.e2 = float4{t.c.x - t.a.x, t.c.y - t.a.y, t.c.z - t.a.z, 0.0f};  // edge2 = c - a
        d.nx = t.custom.x;
        d.ny = t.custom.y;
        d.nz = t.custom.z;
        d.material = t.material;
        td[j] = d;
    }
    r->tri_aee.resize(9 * (size_t)m);
    for (uint32_t j = 0; j < m; j++) {
        const float v[9] = {td[j].a.x, td[j].a.y, td[j].a.z, td[j].e1.x, td[j].e1.y, td[j].e1.z,
                            td[j].e2.x, td[j].e2.y, td[j].e2.z};
        std::copy(v, v + 9, &r->tri_aee[9 * (size_t)j]);
    }
    r->tri_tree_dirty = true;
    r->moments_dirty = true;
    const std::vector<hrt_dev::MatDev> md = pack_materials(mats32, n_mats);
    // The sign-ordered copy (36 B per node) only where a kernel reads it: the heap-top kernels run for heaps of at
    // most 2^24 nodes (launch_frames, tri_small); a larger tree would pay up to ~2.4 GB of host and device memory
    // for nothing
    const bool want_so = n <= (1u << 24);
    bool so_ok = false;
    std::vector<float> so;
    if (want_so) so = pack_nodes_so((const float*)nodes32, n, so_ok);
    else r->nodes_so.release();
    int rc = ensure(r->nodes, 2 * (size_t)std::max<uint32_t>(n, 1));
    if (!rc && want_so) rc = ensure(r->nodes_so, so.size());
    if (!rc) rc = ensure(r->tris, std::max<uint32_t>(m, 1));
    if (!rc) rc = ensure(r->tri_geo, 9 * (size_t)std::max<uint32_t>(m, 1));
    if (!rc) rc = ensure(r->mats, std::max<uint32_t>(n_mats, 1));
    if (rc) return rc;
    if (n) HIP_TRY(hipMemcpyAsync(r->nodes.ptr, nodes32, (size_t)n * 32u, hipMemcpyHostToDevice, r->stream));
    if (want_so)
        HIP_TRY(hipMemcpyAsync(r->nodes_so.ptr, so.data(), so.size() * sizeof(float), hipMemcpyHostToDevice, r->stream));
    if (m) HIP_TRY(hipMemcpyAsync(r->tris.ptr, td.data(), (size_t)m * sizeof(td[0]), hipMemcpyHostToDevice, r->stream));
    if (m)  // (tri_aee: the same a, e1, e2 floats, 9 per triangle)
        HIP_TRY(hipMemcpyAsync(r->tri_geo.ptr, r->tri_aee.data(), r->tri_aee.size() * sizeof(float), hipMemcpyHostToDevice,
                               r->stream));
    if (n_mats)
        HIP_TRY(hipMemcpyAsync(r->mats.ptr, md.data(), (size_t)n_mats * sizeof(md[0]), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->bvh_n = n;
    r->bvh_m = m;
    r->so_ok = so_ok;
    r->dev_geom = false;  // (the heap and tri_aee are back: tri_bvh chooses the walk again)
    r->tb_parent.release();
    return RT_OK;
}

// Triangles from device memory, with an LBVH built for them on the device (include/hrt.h; rt_lbvh.hip, rt_lbvh.hpp).
// Everything is written to the staging buffers and swapped in after the status block says the build is good.
int rt_set_triangles_device(rt_renderer* r, const void* tris64_dev, uint32_t n_tris, const void* mats32, uint32_t n_mats) {
    return rt_set_triangles_device_with(r, tris64_dev, n_tris, mats32, n_mats, RT_TREE_LBVH);
}

// builder: RT_TREE_LBVH (Karras' topology, k_lbvh_topology) or RT_TREE_PLOC (rt_ploc.hip); everything around it is shared.
int rt_set_triangles_device_with(rt_renderer* r, const void* tris64_dev, uint32_t n_tris, const void* mats32, uint32_t n_mats,
                                 uint32_t builder) {
    if (!r) return fail(RT_ERR_ARG, "rt_set_triangles_device: null");
    if (builder != RT_TREE_LBVH && builder != RT_TREE_PLOC)
        return fail(RT_ERR_ARG, "rt_set_triangles_device: unknown builder " + std::to_string(builder));
    if (r->mode == RT_MODE_SPHERE) return fail(RT_ERR_ARG, "rt_set_triangles_device: the sphere program has no triangles");
    if (n_tris && !tris64_dev) return fail(RT_ERR_ARG, "rt_set_triangles_device: null triangles");
    if ((uintptr_t)tris64_dev % 16u) return fail(RT_ERR_ARG, "rt_set_triangles_device: triangles must be 16-byte aligned");
    if (n_tris >= (1u << 26)) return fail(RT_ERR_ARG, "rt_set_triangles_device: 2^26 or more triangles");
    if (n_mats >= (1u << 28)) return fail(RT_ERR_ARG, "rt_set_triangles_device: more than 2^28 materials");
    if (n_mats && !mats32) return fail(RT_ERR_ARG, "rt_set_triangles_device: null materials");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    const std::vector<hrt_dev::MatDev> md = pack_materials(mats32, n_mats);
    const size_t n = n_tris, n1 = std::max<size_t>(n, 1);
    int rc = ensure(r->lb_tris, n1);
    if (!rc) rc = ensure(r->lb_geo, 9 * n1);
    if (!rc) rc = ensure(r->lb_mats, std::max<uint32_t>(n_mats, 1));
    if (!rc) rc = ensure(r->lb_hnodes, 2 * std::max<size_t>(n1 - 1, 1));
    if (!rc) rc = ensure(r->lb_order, n1);
    if (!rc) rc = ensure(r->lb_stat, hrt_lbvh::STAT_WORDS);
    if (rc) return rc;
    uint64_t stat[hrt_lbvh::STAT_WORDS] = {};
    if (n) {
        const size_t tiles = (n + RT_REGROUP_TILE - 1u) / RT_REGROUP_TILE;
        rc = ensure(r->lb_keys, 2 * n);
        if (!rc) rc = ensure(r->lb_parent, 2 * n);
        if (!rc) rc = ensure(r->lb_arrivals, n);
        if (!rc) rc = ensure(r->lb_boxes, 2 * n * hrt_lbvh::BOX_WORDS);
        if (!rc) rc = ensure(r->regroup_entries, 4u * n);
        if (!rc) rc = ensure(r->regroup_counts, 256u * tiles + hrt_regroup::TAIL_WORDS);
        if (rc) return rc;
        hrt_lbvh::Launch a{};
        a.tris64 = tris64_dev;
        a.n = n_tris;
        a.n_mats = n_mats;
        a.tris_out = r->lb_tris.ptr;
        a.geo_out = r->lb_geo.ptr;
        a.hnodes = (hrt_lbvh::U4*)r->lb_hnodes.ptr;
        a.order = r->lb_order.ptr;
        a.keys = r->lb_keys.ptr;
        a.keys_sorted = r->lb_keys.ptr + n;
        a.parent = r->lb_parent.ptr;
        a.arrivals = r->lb_arrivals.ptr;
        a.boxes = r->lb_boxes.ptr;
        a.stat = r->lb_stat.ptr;
        a.sort_entries = r->regroup_entries.ptr;
        a.sort_counts = r->regroup_counts.ptr;
        if (builder == RT_TREE_PLOC) {
            // (pinned host memory: the builder reads a cluster count back per iteration)
            if (!r->refit_stat_host && hipHostMalloc((void**)&r->refit_stat_host, hrt_lbvh::STAT_WORDS * sizeof(uint64_t),
                                                     hipHostMallocDefault) != hipSuccess) {
                r->refit_stat_host = nullptr;
                return fail(RT_ERR_ALLOC, "rt_set_triangles_device: hipHostMalloc of the status block failed");
            }
            HIP_TRY(hrt_launch_lbvh_ploc(a, r->refit_stat_host, r->stream));
        } else {
            HIP_TRY(hrt_launch_lbvh(a, r->stream));
        }
        HIP_TRY(hipMemcpyAsync(stat, r->lb_stat.ptr, sizeof stat, hipMemcpyDeviceToHost, r->stream));
    }
    if (n_mats)
        HIP_TRY(hipMemcpyAsync(r->lb_mats.ptr, md.data(), (size_t)n_mats * sizeof(md[0]), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (stat[7] != 0) return fail(RT_ERR_ARG, "rt_set_triangles_device: triangle material index out of range");
    const uint32_t finite = (uint32_t)stat[6];
    if (finite > n_tris) return fail(RT_ERR_DEVICE, "rt_set_triangles_device: the build's status block is not consistent");
    hrt::TriBvh T;
    T.root_word = hrt_lbvh::root_word(finite);
    T.depth = (uint32_t)stat[8];
    if (finite) {
        double lo[3], hi[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = hrt_lbvh::f64_from_key(~stat[k]);
            hi[k] = hrt_lbvh::f64_from_key(stat[3 + k]);
        }
        hrt_lbvh::root_sphere(lo, hi, T.root_center, &T.root_radius);
    }
    swap_buffers(r->tris, r->lb_tris);
    swap_buffers(r->tri_geo, r->lb_geo);
    swap_buffers(r->mats, r->lb_mats);
    swap_buffers(r->tb_hnodes, r->lb_hnodes);
    swap_buffers(r->tb_order, r->lb_order);
    swap_buffers(r->tb_parent, r->lb_parent);  // (the links belong to the tree: a failed build has not touched the live ones)
    r->tri_tree = std::move(T);
    r->tb_n_nodes = hrt_lbvh::node_slots(finite);
    r->tb_n_order = finite;
    r->tb_builder = builder;
    const bool ploc_nodes = builder == RT_TREE_PLOC && hrt_lbvh::node_slots(finite) != 0u;
    r->tb_iterations = ploc_nodes ? (uint32_t)stat[10] : 0u;
    r->tb_flat = ploc_nodes ? (uint32_t)stat[11] : 0u;
    r->tri_tree_dirty = false;
    r->moments_dirty = true;
    r->dev_geom = true;
    r->dev_n_mats = n_mats;
    r->bvh_n = 0;  // no reference heap: nothing reads one in this state (scene_params: tri_bvh)
    r->bvh_m = n_tris;
    r->so_ok = false;
    r->nodes.release();
    r->nodes_so.release();
    std::vector<float>().swap(r->tri_aee);
    r->cost_learn = true;
    return RT_OK;
}

// The builder on the host (rt_lbvh.hpp host_build): pure CPU, no device.
int rt_host_lbvh_build(const void* tris64, uint32_t n_tris, void* hnodes_out, size_t hnode_cap, uint32_t* order_out,
                       size_t order_cap, uint32_t info[8], float root[4]) {
    return rt_host_lbvh_build_with(tris64, n_tris, RT_TREE_LBVH, hnodes_out, hnode_cap, order_out, order_cap, info, root);
}

int rt_host_lbvh_build_with(const void* tris64, uint32_t n_tris, uint32_t builder, void* hnodes_out, size_t hnode_cap,
                            uint32_t* order_out, size_t order_cap, uint32_t info[8], float root[4]) {
    if (!info || !root) return fail(RT_ERR_ARG, "rt_host_lbvh_build: null info or root");
    if (builder != RT_TREE_LBVH && builder != RT_TREE_PLOC)
        return fail(RT_ERR_ARG, "rt_host_lbvh_build: unknown builder " + std::to_string(builder));
    if (n_tris && !tris64) return fail(RT_ERR_ARG, "rt_host_lbvh_build: null triangles");
    if (n_tris >= (1u << 26)) return fail(RT_ERR_ARG, "rt_host_lbvh_build: 2^26 or more triangles");
    std::vector<float> aee(9 * (size_t)n_tris);
    for (uint32_t j = 0; j < n_tris; j++) {
        hrt::Triangle t;  // (no alignment asked of the caller)
        std::memcpy(&t, (const char*)tris64 + 64u * (size_t)j, sizeof t);
        const float v[9] = {t.a.x, t.a.y, t.a.z, t.b.x - t.a.x, t.b.y - t.a.y, t.b.z - t.a.z,
                            t.c.x - t.a.x, t.c.y - t.a.y, t.c.z - t.a.z};
        std::copy(v, v + 9, &aee[9 * (size_t)j]);
    }
    const hrt_lbvh::HostTree T = hrt_lbvh::host_build(aee.data(), n_tris, builder);
    const size_t nodes = T.hnodes.size() / 2;
    const uint32_t i8[8] = {(uint32_t)nodes, (uint32_t)T.order.size(), T.finite, T.root, T.depth, T.iterations, T.flat, 0u};
    std::copy(i8, i8 + 8, info);
    for (int k = 0; k < 3; k++) root[k] = T.rc[k];
    root[3] = T.radius;
    if (hnode_cap == 0 && order_cap == 0) return RT_OK;
    if (hnode_cap < nodes || order_cap < T.order.size()) return fail(RT_ERR_ARG, "rt_host_lbvh_build: a capacity is too small");
    if ((nodes && !hnodes_out) || (!T.order.empty() && !order_out)) return fail(RT_ERR_ARG, "rt_host_lbvh_build: null output");
    if (nodes) std::memcpy(hnodes_out, T.hnodes.data(), nodes * 32u);
    if (!T.order.empty()) std::memcpy(order_out, T.order.data(), T.order.size() * sizeof(uint32_t));
    return RT_OK;
}

// The device tree's boxes for a moved mesh (include/hrt.h; rt_lbvh.hip k_lbvh_refit_prep / _fit). The topology (tb_order,
// tb_parent, the child words of tb_hnodes) is read and kept; the triangle records and the packed nodes are written to the
// staging set and swapped in after the status block says the refit is good.
int rt_refit_triangles_device(rt_renderer* r, const void* tris64_dev, uint32_t n_tris) {
    if (!r) return fail(RT_ERR_ARG, "rt_refit_triangles_device: null");
    if (r->mode == RT_MODE_SPHERE) return fail(RT_ERR_ARG, "rt_refit_triangles_device: the sphere program has no triangles");
    if (n_tris && !tris64_dev) return fail(RT_ERR_ARG, "rt_refit_triangles_device: null triangles");
    if ((uintptr_t)tris64_dev % 16u) return fail(RT_ERR_ARG, "rt_refit_triangles_device: triangles must be 16-byte aligned");
    if (!r->dev_geom)
        return fail(RT_ERR_STATE, "rt_refit_triangles_device: no device geometry to refit (rt_set_triangles_device first)");
    if (n_tris != r->bvh_m)
        return fail(RT_ERR_ARG, "rt_refit_triangles_device: n_tris = " + std::to_string(n_tris) + ", the tree was built over " +
                                    std::to_string(r->bvh_m) + " triangles");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (n_tris == 0) {  // (an empty tree stays the empty tree)
        r->cost_learn = true;
        return RT_OK;
    }
    const size_t n = n_tris;
    const uint32_t m = r->tb_n_order, slots = hrt_lbvh::node_slots(m);
    if (m > n_tris || (slots && (!r->tb_parent.ptr || r->tb_parent.cap < 2 * n || r->tb_hnodes.cap < 2 * (size_t)slots ||
                                 r->tb_order.cap < m)))
        return fail(RT_ERR_STATE, "rt_refit_triangles_device: the live tree is not consistent");
    int rc = ensure(r->lb_tris, n);
    if (!rc) rc = ensure(r->lb_geo, 9 * n);
    if (!rc) rc = ensure(r->lb_hnodes, 2 * std::max<size_t>(n - 1, 1));
    if (!rc) rc = ensure(r->lb_stat, hrt_lbvh::STAT_WORDS);
    if (!rc && slots) rc = ensure(r->lb_arrivals, n);
    if (!rc && slots) rc = ensure(r->lb_boxes, 2 * n * hrt_lbvh::BOX_WORDS);
    if (rc) return rc;
    hrt_lbvh::Refit a{};
    a.tris64 = tris64_dev;
    a.n = n_tris;
    a.n_mats = r->dev_n_mats;
    a.m = m;
    a.geo_live = r->tri_geo.ptr;
    a.hnodes_live = (const hrt_lbvh::U4*)r->tb_hnodes.ptr;
    a.order = r->tb_order.ptr;
    a.parent = r->tb_parent.ptr;
    a.tris_out = r->lb_tris.ptr;
    a.geo_out = r->lb_geo.ptr;
    a.hnodes = (hrt_lbvh::U4*)r->lb_hnodes.ptr;
    a.arrivals = r->lb_arrivals.ptr;
    a.boxes = r->lb_boxes.ptr;
    a.stat = r->lb_stat.ptr;
    // (pinned host memory: the copy is one asynchronous transfer, not a staged one)
    if (!r->refit_stat_host &&
        hipHostMalloc((void**)&r->refit_stat_host, hrt_lbvh::STAT_WORDS * sizeof(uint64_t), hipHostMallocDefault) != hipSuccess) {
        r->refit_stat_host = nullptr;
        return fail(RT_ERR_ALLOC, "rt_refit_triangles_device: hipHostMalloc of the status block failed");
    }
    uint64_t* const stat = r->refit_stat_host;
    HIP_TRY(hrt_launch_lbvh_refit(a, r->stream));
    HIP_TRY(hipMemcpyAsync(stat, r->lb_stat.ptr, hrt_lbvh::STAT_WORDS * sizeof(uint64_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (stat[7] != 0) return fail(RT_ERR_ARG, "rt_refit_triangles_device: triangle material index out of range");
    if (stat[9] != 0)
        return fail(RT_ERR_ARG, "rt_refit_triangles_device: " + std::to_string(stat[9]) +
                                    " triangles changed between finite and non-finite since the build (build again)");
    if (stat[6] != m) return fail(RT_ERR_DEVICE, "rt_refit_triangles_device: the refit's status block is not consistent");
    if (m) {
        double lo[3], hi[3];
        for (int k = 0; k < 3; k++) {
            lo[k] = hrt_lbvh::f64_from_key(~stat[k]);
            hi[k] = hrt_lbvh::f64_from_key(stat[3 + k]);
        }
        hrt_lbvh::root_sphere(lo, hi, r->tri_tree.root_center, &r->tri_tree.root_radius);
    }
    if (slots) r->tri_tree.depth = (uint32_t)stat[8];
    swap_buffers(r->tris, r->lb_tris);
    swap_buffers(r->tri_geo, r->lb_geo);
    if (slots) swap_buffers(r->tb_hnodes, r->lb_hnodes);
    r->moments_dirty = true;
    r->cost_learn = true;
    return RT_OK;
}

namespace {
void aee_of_triangles(const void* tris64, uint32_t n_tris, std::vector<float>& aee) {
    aee.resize(9 * (size_t)n_tris);
    for (uint32_t j = 0; j < n_tris; j++) {
        hrt::Triangle t;  // (no alignment asked of the caller)
        std::memcpy(&t, (const char*)tris64 + 64u * (size_t)j, sizeof t);
        const float v[9] = {t.a.x, t.a.y, t.a.z, t.b.x - t.a.x, t.b.y - t.a.y, t.b.z - t.a.z,
                            t.c.x - t.a.x, t.c.y - t.a.y, t.c.z - t.a.z};
        std::copy(v, v + 9, &aee[9 * (size_t)j]);
    }
}
}  // namespace

// The refit on the host (rt_lbvh.hpp host_refit: host_build's two halves over two arrays): pure CPU, no device.
int rt_host_lbvh_refit(const void* tris64_topology, const void* tris64, uint32_t n_tris, void* hnodes_out, size_t hnode_cap,
                       uint32_t* order_out, size_t order_cap, uint32_t info[8], float root[4]) {
    return rt_host_lbvh_refit_with(tris64_topology, tris64, n_tris, RT_TREE_LBVH, hnodes_out, hnode_cap, order_out, order_cap, info,
                                   root);
}

int rt_host_lbvh_refit_with(const void* tris64_topology, const void* tris64, uint32_t n_tris, uint32_t builder, void* hnodes_out,
                            size_t hnode_cap, uint32_t* order_out, size_t order_cap, uint32_t info[8], float root[4]) {
    if (!info || !root) return fail(RT_ERR_ARG, "rt_host_lbvh_refit: null info or root");
    if (builder != RT_TREE_LBVH && builder != RT_TREE_PLOC)
        return fail(RT_ERR_ARG, "rt_host_lbvh_refit: unknown builder " + std::to_string(builder));
    if (n_tris && (!tris64_topology || !tris64)) return fail(RT_ERR_ARG, "rt_host_lbvh_refit: null triangles");
    if (n_tris >= (1u << 26)) return fail(RT_ERR_ARG, "rt_host_lbvh_refit: 2^26 or more triangles");
    std::vector<float> aee_t, aee;
    aee_of_triangles(tris64_topology, n_tris, aee_t);
    aee_of_triangles(tris64, n_tris, aee);
    hrt_lbvh::HostTree T;
    if (!hrt_lbvh::host_refit(aee_t.data(), aee.data(), n_tris, T, builder))
        return fail(RT_ERR_ARG, "rt_host_lbvh_refit: a triangle is finite in one array and not in the other");
    const size_t nodes = T.hnodes.size() / 2;
    const uint32_t i8[8] = {(uint32_t)nodes, (uint32_t)T.order.size(), T.finite, T.root, T.depth, T.iterations, T.flat, 0u};
    std::copy(i8, i8 + 8, info);
    for (int k = 0; k < 3; k++) root[k] = T.rc[k];
    root[3] = T.radius;
    if (hnode_cap == 0 && order_cap == 0) return RT_OK;
    if (hnode_cap < nodes || order_cap < T.order.size()) return fail(RT_ERR_ARG, "rt_host_lbvh_refit: a capacity is too small");
    if ((nodes && !hnodes_out) || (!T.order.empty() && !order_out)) return fail(RT_ERR_ARG, "rt_host_lbvh_refit: null output");
    if (nodes) std::memcpy(hnodes_out, T.hnodes.data(), nodes * 32u);
    if (!T.order.empty()) std::memcpy(order_out, T.order.data(), T.order.size() * sizeof(uint32_t));
    return RT_OK;
}

// The tree cost on the host (rt_lbvh.hpp host_cost): a pure function of the node bytes.
int rt_host_lbvh_cost(const void* hnodes, size_t node_slots, uint32_t root_word, uint64_t cost[4]) {
    if (!cost) return fail(RT_ERR_ARG, "rt_host_lbvh_cost: null cost");
    for (int k = 0; k < 4; k++) cost[k] = 0;
    if ((root_word & hrt_lbvh::LEAF_BIT) != 0u) return RT_OK;  // a tree without nodes
    if (root_word >= node_slots) return fail(RT_ERR_ARG, "rt_host_lbvh_cost: the root word names a node past node_slots");
    if (!hnodes) return fail(RT_ERR_ARG, "rt_host_lbvh_cost: null nodes");
    std::vector<hrt_lbvh::U4> nodes(2 * node_slots);  // (no alignment asked of the caller)
    std::memcpy(nodes.data(), hnodes, node_slots * 32u);
    hrt_lbvh::host_cost(nodes.data(), node_slots, root_word, cost);
    return RT_OK;
}

// The same read-out of the tree the renderer walks (rt_lbvh.hip k_tri_tree_cost). Blocking; the four words are summed in
// the status block's cost words, which no draw reads.
int rt_get_tri_tree_cost(rt_renderer* r, uint64_t cost[4]) {
    if (!r || !cost) return fail(RT_ERR_ARG, "rt_get_tri_tree_cost: null");
    if (int rc = need_tri_tree(r, "rt_get_tri_tree_cost", true)) return rc;
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (int rc = upload_tri_tree(r)) return rc;  // (a host tree not built yet)
    for (int k = 0; k < 4; k++) cost[k] = 0;
    const uint32_t root = r->tri_tree.root_word, slots = r->tb_n_nodes;
    if ((root & hrt_lbvh::LEAF_BIT) != 0u || slots == 0u) return RT_OK;
    if (root >= slots || r->tb_hnodes.cap < 2 * (size_t)slots)
        return fail(RT_ERR_STATE, "rt_get_tri_tree_cost: the tree is not consistent");
    if (int rc = ensure(r->lb_stat, hrt_lbvh::STAT_WORDS)) return rc;
    uint64_t* const words = r->lb_stat.ptr + 12;
    HIP_TRY(hrt_launch_tri_tree_cost(r->tb_hnodes.ptr, slots, root, words, r->stream));
    HIP_TRY(hipMemcpyAsync(cost, words, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return RT_OK;
}

// What the renderer walks, in numbers (include/hrt.h). A host SAH tree not built yet is built first.
int rt_get_tri_tree_info(rt_renderer* r, uint32_t info[8]) {
    if (!r || !info) return fail(RT_ERR_ARG, "rt_get_tri_tree_info: null");
    if (int rc = need_tri_tree(r, "rt_get_tri_tree_info")) return rc;
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (int rc = upload_tri_tree(r)) return rc;
    const bool dev = r->dev_geom;
    const uint32_t i8[8] = {dev ? r->tb_builder : RT_TREE_HOST_SAH, r->tb_n_nodes, r->tb_n_order, r->tri_tree.root_word,
                            r->tri_tree.depth, dev ? r->tb_iterations : 0u, dev ? r->tb_flat : 0u, 0u};
    std::copy(i8, i8 + 8, info);
    return RT_OK;
}

int rt_testing_get_tri_tree(rt_renderer* r, void* hnodes_out, size_t hnode_cap, uint32_t* order_out, size_t order_cap,
                            uint32_t info[8], float root[4]) {
    if (!r || !info || !root) return fail(RT_ERR_ARG, "rt_testing_get_tri_tree: null");
    if (int rc = need_tri_tree(r, "rt_testing_get_tri_tree", true)) return rc;
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (int rc = upload_tri_tree(r)) return rc;  // (a host tree not built yet)
    const hrt::TriBvh& T = r->tri_tree;
    const size_t nodes = r->tb_n_nodes, leaves = r->tb_n_order;
    const bool dev = r->dev_geom;  // (the two PLOC counts, as rt_host_lbvh_build_with reports them)
    const uint32_t i8[8] = {(uint32_t)nodes, (uint32_t)leaves, (uint32_t)leaves, T.root_word, T.depth, dev ? r->tb_iterations : 0u,
                            dev ? r->tb_flat : 0u, 0u};
    std::copy(i8, i8 + 8, info);
    for (int k = 0; k < 3; k++) root[k] = T.root_center[k];
    root[3] = T.root_radius;
    if (hnode_cap == 0 && order_cap == 0) return RT_OK;
    if (hnode_cap < nodes || order_cap < leaves) return fail(RT_ERR_ARG, "rt_testing_get_tri_tree: a capacity is too small");
    if ((nodes && !hnodes_out) || (leaves && !order_out)) return fail(RT_ERR_ARG, "rt_testing_get_tri_tree: null output");
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (nodes) HIP_TRY(hipMemcpy(hnodes_out, r->tb_hnodes.ptr, nodes * 32u, hipMemcpyDeviceToHost));
    if (leaves) HIP_TRY(hipMemcpy(order_out, r->tb_order.ptr, leaves * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_host_check_bvh_sizes(const uint32_t sizes[2], uint32_t n_nodes, uint32_t n_tris, uint32_t n_mats) {
    if (!sizes) return fail(RT_ERR_ARG, "rt_set_bvh: null sizes");
    const uint32_t n = sizes[0], m = sizes[1];
    // The kernel reads nodes[i] for i < n and triangles[j] for j < m only; validate so it cannot fault.
    if (n_nodes < n || n_tris < m) return fail(RT_ERR_ARG, "rt_set_bvh: sizes exceed the buffers given");
    // Tree::build (tree.rs:38) makes n = m.next_power_of_two() (>= 1); the walks rely on it (leaf pairs: the
    // children of nodes n/2 .. n-1 are leaves)
    if (n == 0 || (n & (n - 1u)) != 0) return fail(RT_ERR_ARG, "rt_set_bvh: sizes[0] must be a power of two");
    // The walks load nodes (32 B) and triangles (64 B) through buffer descriptors with 32-bit byte sizes and
    // offsets (rt_kernels.hip node_hit_top, tri_test<TBUF>): n x 32 and m x 64 must stay below 2^32.
    if (n > RT_MAX_TREE_NODES) return fail(RT_ERR_ARG, "rt_set_bvh: more than RT_MAX_TREE_NODES (2^26) nodes");
    if (m >= (1u << 26)) return fail(RT_ERR_ARG, "rt_set_bvh: 2^26 or more triangles");
    if (n_mats >= (1u << 28)) return fail(RT_ERR_ARG, "rt_set_bvh: more than 2^28 materials");
    return RT_OK;
}

int rt_testing_set_faults(rt_renderer* r, uint32_t ring_slots_max, uint32_t fail_alloc_above_mb) {
    if (!r) return fail(RT_ERR_ARG, "rt_testing_set_faults: null");
    r->test_ring_slots_max = ring_slots_max;
    r->test_fail_alloc_above_mb = fail_alloc_above_mb;
    return RT_OK;
}

int rt_testing_get_tile_order(rt_renderer* r, uint32_t* sum_out, uint32_t* order_out, size_t cap, size_t* count) {
    if (!r || !count) return fail(RT_ERR_ARG, "rt_testing_get_tile_order: null");
    const size_t n = r->order_tiles;
    *count = n;
    if (cap == 0u || n == 0u) return RT_OK;
    if (cap < n || !sum_out || !order_out) return fail(RT_ERR_ARG, "rt_testing_get_tile_order: the capacity is too small");
    HIP_TRY(hipMemcpyAsync(sum_out, r->tile_sum.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipMemcpyAsync(order_out, r->tile_order.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return RT_OK;
}

int rt_testing_set_descent_hold(rt_renderer* r, uint32_t hold) {
    if (hold > 64) return fail(RT_ERR_ARG, "rt_testing_set_descent_hold: hold must be 0..64");
    if (!r) return fail(RT_ERR_ARG, "rt_testing_set_descent_hold: null");
    r->descent_hold = hold;
    return RT_OK;
}

int rt_testing_set_tile_lists(rt_renderer* r, uint32_t mode, uint32_t k) {
    if (mode > 2u || k > hrt_tiles::K_MAX) return fail(RT_ERR_ARG, "rt_testing_set_tile_lists: mode must be 0..2 and k 0..8");
    if (!r) return fail(RT_ERR_ARG, "rt_testing_set_tile_lists: null");
    r->tile_list_mode = mode;
    r->tile_list_k = k;
    return RT_OK;
}

int rt_testing_get_tile_lists_resolved(rt_renderer* r, uint64_t* blocks) {
    if (!r || !blocks) return fail(RT_ERR_ARG, "rt_testing_get_tile_lists_resolved: null");
    const int rc = finish_stats(r);
    if (rc) return rc;
    *blocks = r->blocks_resolved;
    return RT_OK;
}

int rt_testing_get_tile_lists(rt_renderer* r, uint32_t* words_out, size_t cap, size_t* count) {
    if (!r || !count) return fail(RT_ERR_ARG, "rt_testing_get_tile_lists: null");
    if (r->mode != RT_MODE_SPHERE) return fail(RT_ERR_ARG, "rt_testing_get_tile_lists: the sphere program only");
    if (!r->has_camera) return fail(RT_ERR_STATE, "rt_set_camera must be called before rt_testing_get_tile_lists");
    DeviceScope scope(r->device);
    if (scope.rc) return scope.rc;
    hrt_dev::KParams P{};
    int rc = scene_params(r, P);
    if (rc) return rc;
    const hrt_tiles::View V = tile_view_of(P, r->tile_list_k);
    const size_t n = (size_t)V.tiles_w * V.tiles_h * hrt_tiles::WORDS;
    *count = n;
    if (cap == 0) return RT_OK;
    if (cap < n || !words_out) return fail(RT_ERR_ARG, "rt_testing_get_tile_lists: the capacity is too small");
    if (n == 0) return RT_OK;
    rc = ensure_tile_lists(r, P);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(words_out, r->tile_lists.ptr, n * sizeof(uint32_t), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return RT_OK;
}

int rt_host_tile_lists(const void* camera80, uint32_t width, uint32_t height, uint32_t row0, uint32_t row_step,
                       uint32_t row_block, const void* spheres48, uint32_t n, uint32_t min_sphere_slots, uint32_t k,
                       uint32_t* words_out, size_t cap, size_t* count) {
    if (!camera80 || !count || (n && !spheres48)) return fail(RT_ERR_ARG, "rt_host_tile_lists: null");
    if (width == 0 || height == 0 || row_step == 0 || k > hrt_tiles::K_MAX)
        return fail(RT_ERR_ARG, "rt_host_tile_lists: width, height and row_step must be positive and k at most 8");
    // the renderer's own steps: the slots and their culling BVH (upload_spheres), the camera constants (scene_params)
    const hrt::Sphere* sp = (const hrt::Sphere*)spheres48;
    const uint32_t nslots = std::max(n, min_sphere_slots);
    std::vector<float> cr(4 * (size_t)nslots, 0.0f);
    for (uint32_t i = 0; i < n; i++) {
        cr[4 * i + 0] = sp[i].center.x;
        cr[4 * i + 1] = sp[i].center.y;
        cr[4 * i + 2] = sp[i].center.z;
        cr[4 * i + 3] = sp[i].radius;
    }
    const hrt::SphereBvh B = hrt::build_sphere_bvh(cr);
    hrt::Camera c;
    std::memcpy(&c, camera80, sizeof c);
    hrt_dev::KParams P{};
    const float* cam = &c.eye.x;
    for (int i = 0; i < 4; i++) {
        P.cam.eye[i] = cam[i];
        P.cam.dir[i] = cam[4 + i];
        P.cam.up[i] = cam[8 + i];
        P.cam.right[i] = cam[12 + i];
    }
    P.cam.focal = c.params.x;
    P.cam.blur = c.params.y;
    P.cam.k = std::tan(c.params.z * 0.5f);
    P.cam.aspect = (float)width / (float)height;
    P.cam.wm1 = (float)width - 1.0f;
    P.cam.hm1 = (float)height - 1.0f;
    P.W = width;
    P.H = height;
    P.row0 = row0;
    P.row_block = std::max(row_block, 1u);
    P.row_stride = row_step * P.row_block;
    P.nrows = local_rows_of(height, row0, row_step, P.row_block);
    const hrt_tiles::View V = tile_view_of(P, k);
    const size_t ntiles = (size_t)V.tiles_w * V.tiles_h, words = ntiles * hrt_tiles::WORDS;
    *count = words;
    if (cap == 0) return RT_OK;
    if (cap < words || !words_out) return fail(RT_ERR_ARG, "rt_host_tile_lists: the capacity is too small");
    for (size_t t = 0; t < ntiles; t++)
        hrt_tiles::tile_list(V, (uint32_t)t, B.sph.data(), (uint32_t)B.slot.size(), words_out + t * hrt_tiles::WORDS);
    return RT_OK;
}

int rt_testing_set_trace_rays_per_lane(rt_renderer* r, uint32_t rays_per_lane) {
    if (rays_per_lane > 64) return fail(RT_ERR_ARG, "rt_testing_set_trace_rays_per_lane: rays_per_lane must be 0..64");
    if (!r) return fail(RT_ERR_ARG, "rt_testing_set_trace_rays_per_lane: null");
    r->trace_rays_per_lane = rays_per_lane;
    return RT_OK;
}

int rt_set_time(rt_renderer* r, uint32_t time) {
    if (!r) return fail(RT_ERR_ARG, "rt_set_time: null");
    r->time = time;
    return RT_OK;
}

int rt_set_frame_count(rt_renderer* r, uint32_t fc) {
    if (!r) return fail(RT_ERR_ARG, "rt_set_frame_count: null");
    r->frame_count = fc;
    return RT_OK;
}

int rt_get_frame_count(const rt_renderer* r, uint32_t* out) {
    if (!r || !out) return fail(RT_ERR_ARG, "rt_get_frame_count: null");
    *out = r->frame_count;
    return RT_OK;
}

int rt_draw(rt_renderer* r) {
    if (!r) return fail(RT_ERR_ARG, "rt_draw: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    return launch_frames(r, 1, r->time, 0);
}

int rt_draw_frames(rt_renderer* r, uint32_t count, uint32_t time0, uint32_t dtime) {
    if (!r) return fail(RT_ERR_ARG, "rt_draw_frames: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (count == 0) return RT_OK;
    int rc = launch_frames(r, count, time0, dtime);
    if (!rc) r->time = time0 + (count - 1) * dtime;
    return rc;
}

// Ray queries (include/hrt.h): the scene as a tiles draw would see it (scene_params: variant, tri_bvh, min_sphere_slots),
// none of the draw's state — no image, counters, stats, frame count or cost order is read or written.
int rt_cast_rays(rt_renderer* r, const void* origins_dev, const void* dirs_dev, uint32_t n, void* hits_dev) {
    if (!r) return fail(RT_ERR_ARG, "rt_cast_rays: null");
    if (n == 0) return RT_OK;
    if (!origins_dev || !dirs_dev || !hits_dev) return fail(RT_ERR_ARG, "rt_cast_rays: null buffer");
    if (misaligned(16, {hits_dev}) || misaligned(4, {origins_dev, dirs_dev}))
        return fail(RT_ERR_ARG, "rt_cast_rays: hits must be 16-byte aligned, origins and directions 4-byte aligned");
    static_assert(sizeof(rt_hit) == 32, "rt_hit: two 16-byte stores per record (k_cast_rays)");
    QueryScope q(r);
    if (q.rc) return q.rc;
    HIP_TRY(hrt_launch_cast(r->mode, q.variant, q.P, (const float*)origins_dev, (const float*)dirs_dev, n, hits_dev, r->stream));
    return RT_OK;
}

int rt_occluded(rt_renderer* r, const void* origins_dev, const void* dirs_dev, const void* tmax_dev, uint32_t n,
                void* occluded_dev) {
    if (!r) return fail(RT_ERR_ARG, "rt_occluded: null");
    if (n == 0) return RT_OK;
    if (!origins_dev || !dirs_dev || !occluded_dev) return fail(RT_ERR_ARG, "rt_occluded: null buffer");
    if (misaligned(4, {origins_dev, dirs_dev, tmax_dev}))
        return fail(RT_ERR_ARG, "rt_occluded: origins, directions and tmax must be 4-byte aligned");
    QueryScope q(r);
    if (q.rc) return q.rc;
    HIP_TRY(hrt_launch_occluded(r->mode, q.variant, q.P, (const float*)origins_dev, (const float*)dirs_dev,
                                (const float*)tmax_dev, n, occluded_dev, r->stream));
    return RT_OK;
}

// Rays per lane of k_radiance_rays (R; a wave owns 64 R consecutive rays): the largest of 4, 2, 1 that still leaves 48
// waves per compute unit — two full rounds at the kernel's 6 waves per SIMD. A lane with several rays takes the next one
// when a path ends instead of idling behind the wave's longest, but each doubling halves the waves and pulls the lanes
// of a wave apart (their rays are 64 apart, and no longer on the same bounce). Measured on C3's primary rays with 50
// bounces, in pixel order / permuted, as ms per call (DESIGN.md §7c Radiance queries): 0.92 M rays R = 1: 0.56 / 0.72,
// R = 2 (28 waves per CU): 0.70 / 0.68; 2.07 M rays R = 1: 0.93 / 1.30, R = 2 (63 per CU): 0.86 / 1.09, R = 4 (32):
// 0.88 / 1.03; 3.69 M rays R = 2: 1.23 / 1.69, R = 4 (56): 1.21 / 1.50; 8.29 M rays R = 4: 2.28 / 2.96, R = 8 (63):
// 2.34 / 2.69 — 8 never won on both orders.
static uint32_t trace_rays_per_lane(const rt_renderer* r, uint32_t n) {
    if (r->trace_rays_per_lane) return r->trace_rays_per_lane;
    const uint64_t waves_wanted = 48ull * std::max(r->cus, 1u);
    uint32_t R = 4;
    while (R > 1 && (uint64_t)n < 64ull * R * waves_wanted) R >>= 1;
    return R;
}

int rt_trace_rays(rt_renderer* r, const void* origins_dev, const void* dirs_dev, const void* rng_dev, uint32_t seed, uint32_t n,
                  void* radiance_dev, void* queries_dev) {
    if (!r) return fail(RT_ERR_ARG, "rt_trace_rays: null");
    if (n == 0) return RT_OK;
    if (!origins_dev || !dirs_dev || !radiance_dev) return fail(RT_ERR_ARG, "rt_trace_rays: null buffer");
    if (misaligned(4, {origins_dev, dirs_dev, rng_dev, radiance_dev, queries_dev}))
        return fail(RT_ERR_ARG, "rt_trace_rays: origins, directions, states, radiance and queries must be 4-byte aligned");
    QueryScope q(r);
    if (q.rc) return q.rc;
    q.P.bounces = r->params.bounces;
    HIP_TRY(hrt_launch_trace_rays(r->mode, q.variant, q.P, (const float*)origins_dev, (const float*)dirs_dev,
                                  (const uint32_t*)rng_dev, seed, n, trace_rays_per_lane(r, n), (float*)radiance_dev,
                                  (uint32_t*)queries_dev, r->stream));
    return RT_OK;
}

// One path step in the caller's buffers (include/hrt.h rt_bounce): *count_out is zeroed on the stream, then k_bounce_rays.
int rt_bounce_rays(rt_renderer* r, const rt_bounce* io, uint32_t n) {
    if (!r) return fail(RT_ERR_ARG, "rt_bounce_rays: null");
    if (n == 0) return RT_OK;
    if (!io) return fail(RT_ERR_ARG, "rt_bounce_rays: null io");
    if (!io->origins_dev || !io->dirs_dev || !io->rng_dev) return fail(RT_ERR_ARG, "rt_bounce_rays: null buffer");
    if (io->reserved != 0) return fail(RT_ERR_ARG, "rt_bounce_rays: reserved must be 0");
    if (io->index_out_dev && !io->count_out_dev) return fail(RT_ERR_ARG, "rt_bounce_rays: index_out needs count_out");
    if (io->count_out_dev && io->count_out_dev == io->count_in_dev)
        return fail(RT_ERR_ARG, "rt_bounce_rays: count_out must not be count_in");
    if (!io->index_in_dev && n > io->paths) return fail(RT_ERR_ARG, "rt_bounce_rays: n exceeds paths without index_in");
    if (misaligned(16, {io->hits_dev})) return fail(RT_ERR_ARG, "rt_bounce_rays: hits must be 16-byte aligned");
    if (misaligned(4, {io->origins_dev, io->dirs_dev, io->rng_dev, io->throughput_dev, io->queries_dev, io->index_in_dev,
                       io->count_in_dev, io->index_out_dev, io->count_out_dev}))
        return fail(RT_ERR_ARG, "rt_bounce_rays: every buffer but hits must be 4-byte aligned");
    static_assert(sizeof(rt_bounce) == 88, "rt_bounce: ten pointers and two words (hrt/_lib.py RtBounce)");
    QueryScope q(r);
    if (q.rc) return q.rc;
    hrt_dev::BounceIO B{};
    B.origins = (float*)io->origins_dev;
    B.dirs = (float*)io->dirs_dev;
    B.rng = (uint32_t*)io->rng_dev;
    B.throughput = (float*)io->throughput_dev;
    B.queries = (uint32_t*)io->queries_dev;
    B.hits = io->hits_dev;
    B.index_in = (const uint32_t*)io->index_in_dev;
    B.count_in = (const uint32_t*)io->count_in_dev;
    B.index_out = (uint32_t*)io->index_out_dev;
    B.count_out = (uint32_t*)io->count_out_dev;
    B.paths = io->paths;
    if (B.count_out) HIP_TRY(hipMemsetAsync(B.count_out, 0, sizeof(uint32_t), r->stream));
    HIP_TRY(hrt_launch_bounce(r->mode, q.variant, q.P, B, n, r->stream));
    return RT_OK;
}

// Regrouping (include/hrt.h rt_regroup): the key pass and the radix sort of rt_regroup.hip in the renderer's own scratch.
// No scene, camera or draw state is read.
// The point query (include/hrt.h; rt_closest.hip k_closest_points, rt_closest.hpp the function and the definition). Like
// the ray queries it reads the scene through scene_params and nothing of a draw's state.
int rt_closest_points(rt_renderer* r, const void* points_dev, const void* maxd2_dev, uint32_t n, void* out_dev) {
    if (!r) return fail(RT_ERR_ARG, "rt_closest_points: null");
    if (n == 0) return RT_OK;
    if (!points_dev || !out_dev) return fail(RT_ERR_ARG, "rt_closest_points: null buffer");
    if (misaligned(16, {out_dev}) || misaligned(4, {points_dev, maxd2_dev}))
        return fail(RT_ERR_ARG, "rt_closest_points: out must be 16-byte aligned, points and maxd2 4-byte aligned");
    static_assert(sizeof(rt_closest) == 32, "rt_closest: two 16-byte stores per record (k_closest_points)");
    QueryScope q(r, "rt_closest_points");
    if (q.rc) return q.rc;
    hrt_closest::Launch a{};
    tree_fields(a, q.P);
    a.points = (const float*)points_dev;
    a.maxd2 = (const float*)maxd2_dev;
    a.out = out_dev;
    a.n = n;
    if (int rc = r->closest_count.arm(4, r->stream, &a.counts)) return rc;
    HIP_TRY(hrt_launch_closest(a, r->closest_count.on, r->stream));
    return RT_OK;
}

// The definition on the host (rt_closest.hpp host_closest): pure CPU, no device.
int rt_host_closest_points(const void* tris64, uint32_t n_tris, const float* points, const float* maxd2, uint32_t n,
                           void* out32) {
    if (n_tris && !tris64) return fail(RT_ERR_ARG, "rt_host_closest_points: null triangles");
    if (n && (!points || !out32)) return fail(RT_ERR_ARG, "rt_host_closest_points: null points or out");
    std::vector<float> aee;
    aee_of_triangles(tris64, n_tris, aee);
    std::vector<hrt_closest::Record> out(n);
    hrt_closest::host_closest(aee.data(), n_tris, points, maxd2, n, out.data());
    if (n) std::memcpy(out32, out.data(), (size_t)n * sizeof(hrt_closest::Record));
    return RT_OK;
}

// The counting instantiations' switches and read-outs (include/hrt_testing.h), one CounterSlot each.
static int set_counting(rt_renderer* r, CounterSlot rt_renderer::*slot, uint32_t on, const char* who) {
    if (!r) return fail(RT_ERR_ARG, std::string(who) + ": null");
    (r->*slot).on = on != 0u;
    return RT_OK;
}
static int get_counts(rt_renderer* r, CounterSlot rt_renderer::*slot, uint64_t* out, size_t words, const char* who) {
    if (!r || !out) return fail(RT_ERR_ARG, std::string(who) + ": null");
    return (r->*slot).read(r->device, r->stream, out, words);
}

int rt_testing_set_closest_count(rt_renderer* r, uint32_t on) {
    return set_counting(r, &rt_renderer::closest_count, on, "rt_testing_set_closest_count");
}
int rt_testing_get_closest_counts(rt_renderer* r, uint64_t out[4]) {
    return get_counts(r, &rt_renderer::closest_count, out, 4, "rt_testing_get_closest_counts");
}
int rt_testing_set_winding_count(rt_renderer* r, uint32_t on) {
    return set_counting(r, &rt_renderer::winding_count, on, "rt_testing_set_winding_count");
}
int rt_testing_get_winding_counts(rt_renderer* r, uint64_t out[5]) {
    return get_counts(r, &rt_renderer::winding_count, out, 5, "rt_testing_get_winding_counts");
}
int rt_testing_set_multihit_count(rt_renderer* r, uint32_t on) {
    return set_counting(r, &rt_renderer::multihit_count, on, "rt_testing_set_multihit_count");
}
int rt_testing_get_multihit_counts(rt_renderer* r, uint64_t out[4]) {
    return get_counts(r, &rt_renderer::multihit_count, out, 4, "rt_testing_get_multihit_counts");
}
int rt_testing_set_overlap_count(rt_renderer* r, uint32_t on) {
    return set_counting(r, &rt_renderer::overlap_count, on, "rt_testing_set_overlap_count");
}
int rt_testing_get_overlap_counts(rt_renderer* r, uint64_t out[4]) {
    return get_counts(r, &rt_renderer::overlap_count, out, 4, "rt_testing_get_overlap_counts");
}

// ---- winding numbers (include/hrt.h; rt_winding.hip k_winding / k_tree_moments, rt_winding.hpp the function) ----
namespace {
// The moments of the live tree in tb_moments, made when something changed the tree since they were made last. Device
// geometry: the climb over tb_parent in the build's scratch (arrival counters and box slots; nothing a build or a refit
// keeps between calls). The host SAH tree has no parent links on the device: the host mirror's records are uploaded.
int ensure_moments(rt_renderer* r) {
    if (!r->moments_dirty && r->tb_moments.ptr) return RT_OK;
    const uint32_t slots = r->tb_n_nodes, root = r->tri_tree.root_word;
    if ((root & hrt_winding::LEAF_BIT) != 0u || slots == 0u) {  // a tree without nodes: the flat definition answers
        r->moments_dirty = false;
        return ensure(r->tb_moments, hrt_winding::REC_FLOATS);
    }
    if (root >= slots || r->tb_hnodes.cap < 2 * (size_t)slots)
        return fail(RT_ERR_STATE, "rt_winding_numbers: the tree is not consistent");
    if (int rc = ensure(r->tb_moments, hrt_winding::REC_FLOATS * (size_t)slots)) return rc;
    if (r->dev_geom) {
        if (!r->tb_parent.ptr || r->tb_parent.cap < slots)
            return fail(RT_ERR_STATE, "rt_winding_numbers: the device tree has no parent links");
        int rc = ensure(r->lb_arrivals, slots);
        if (!rc) rc = ensure(r->lb_boxes, 2 * (size_t)slots * hrt_winding::SUM_WORDS);
        if (rc) return rc;
        hrt_winding::MomentsLaunch a{};
        a.hnodes = (const hrt_lbvh::U4*)r->tb_hnodes.ptr;
        a.order = r->tb_order.ptr;
        a.geo = r->tri_geo.ptr;
        a.parent = r->tb_parent.ptr;
        a.slots = slots;
        for (int k = 0; k < 3; k++) a.rc[k] = r->tri_tree.root_center[k];
        a.sums = (unsigned long long*)r->lb_boxes.ptr;
        a.arrivals = r->lb_arrivals.ptr;
        a.moments = r->tb_moments.ptr;
        HIP_TRY(hrt_launch_tree_moments(a, r->stream));
    } else {
        const std::vector<uint4> hpacked = pack_bvh_hnodes(r->tri_tree.nodes, r->tri_tree.root_center);
        hrt_winding::Tree T{};
        T.hnodes = (const hrt_lbvh::U4*)hpacked.data();
        T.order = r->tri_tree.order.data();
        T.geo = r->tri_aee.data();
        T.m = (uint32_t)(r->tri_aee.size() / 9);
        T.root = root;
        for (int k = 0; k < 3; k++) T.rc[k] = r->tri_tree.root_center[k];
        std::vector<float> rec(hrt_winding::REC_FLOATS * (size_t)slots);
        if (hpacked.size() < 2 * (size_t)slots || !hrt_winding::host_moments(T, slots, r->tri_tree.order.size(), rec.data()))
            return fail(RT_ERR_STATE, "rt_winding_numbers: the host tree is not consistent");
        HIP_TRY(hipMemcpyAsync(r->tb_moments.ptr, rec.data(), rec.size() * sizeof(float), hipMemcpyHostToDevice, r->stream));
        HIP_TRY(hipStreamSynchronize(r->stream));  // (rec leaves scope)
    }
    r->moments_dirty = false;
    return RT_OK;
}
}  // namespace

}  // extern "C" (HostTree has a template member)

namespace {
// The tree argument of the host mirrors (rt_host_tree_moments, rt_host_winding_numbers, rt_host_cast_rays_multi,
// rt_host_overlap_volumes), copied (no alignment asked of the caller) and checked as far as a size can be; whether the
// nodes are a tree is the caller's to judge (host_moments, host_tree_ok). The mirrors do not refuse the same calls, and
// each keeps its rules:
//   strict   (multi-hit, volumes) the root is always read and the root word passed on; nodes and node_slots must agree;
//            order is read only with nodes.
//   lenient  (winding) without nodes nothing of the tree is read, not even the root: the root word is LEAF_BIT; order is
//            copied whenever it is given; a root word past node_slots is refused here.
struct HostTree {
    std::vector<float> aee;
    std::vector<hrt_lbvh::U4> nodes;
    std::vector<uint32_t> ord;
    uint32_t m = 0, root_word = hrt_lbvh::LEAF_BIT;
    float rc3[3] = {0.0f, 0.0f, 0.0f}, rr_h = 0.0f;
    int rc = RT_OK;
    HostTree(const char* who, bool strict, const void* tris64, uint32_t n_tris, const void* hnodes, size_t node_slots,
             const uint32_t* order, size_t n_order, uint32_t word, const float root[4]) {
        const std::string w(who);
        if (n_tris && !tris64) rc = fail(RT_ERR_ARG, w + ": null triangles");
        else if (strict && !root) rc = fail(RT_ERR_ARG, w + ": null root");
        else if (strict && (node_slots != 0) != (hnodes != nullptr)) rc = fail(RT_ERR_ARG, w + ": nodes and node_slots disagree");
        else if (!strict && node_slots && (!hnodes || !root)) rc = fail(RT_ERR_ARG, w + ": null nodes or root");
        else if ((!strict || node_slots) && n_order && !order) rc = fail(RT_ERR_ARG, w + ": null order");
        else if (node_slots >= (1u << 26) || n_order > (1u << 26)) rc = fail(RT_ERR_ARG, w + ": 2^26 or more node slots or positions");
        else if (!strict && node_slots && (word & hrt_lbvh::LEAF_BIT) == 0u && word >= node_slots)
            rc = fail(RT_ERR_ARG, w + ": the root word names a node past node_slots");
        if (rc) return;
        aee_of_triangles(tris64, n_tris, aee);
        m = n_tris;
        nodes.resize(2 * node_slots);
        if (node_slots) std::memcpy(nodes.data(), hnodes, node_slots * 32u);
        if ((!strict || node_slots) && n_order) ord.assign(order, order + n_order);
        if (strict || node_slots) {
            root_word = word;
            for (int k = 0; k < 3; k++) rc3[k] = root[k];
            rr_h = std::nextafter(root[3] * (1.0f + 0x1p-9f), INFINITY);  // (scene_params: tb_rr_h)
        }
    }
    template <typename T>
    void fields(T& t) const {
        t.hnodes = nodes.data();
        t.order = ord.data();
        t.geo = aee.data();
        t.m = m;
        t.root = root_word;
        for (int k = 0; k < 3; k++) t.rc[k] = rc3[k];
        t.rr_h = rr_h;
    }
};
}  // namespace

extern "C" {

int rt_winding_numbers(rt_renderer* r, const void* points_dev, uint32_t n, float beta, void* w_dev) {
    if (!r) return fail(RT_ERR_ARG, "rt_winding_numbers: null");
    if (n == 0) return RT_OK;
    if (!points_dev || !w_dev) return fail(RT_ERR_ARG, "rt_winding_numbers: null buffer");
    if (misaligned(4, {points_dev, w_dev})) return fail(RT_ERR_ARG, "rt_winding_numbers: points and w must be 4-byte aligned");
    if (!hrt_winding::beta_ok(beta))
        return fail(RT_ERR_ARG, "rt_winding_numbers: beta must be 0 (the default 2.0) or at least 1 (+inf: no dipoles)");
    QueryScope q(r, "rt_winding_numbers");
    if (q.rc) return q.rc;
    if (int rc = ensure_moments(r)) return rc;
    hrt_winding::Launch a{};
    tree_fields(a.tree, q.P);
    a.tree.moments = r->tb_moments.ptr;
    a.points = (const float*)points_dev;
    a.out = (float*)w_dev;
    a.n = n;
    a.beta = beta;
    if (int rc = r->winding_count.arm(5, r->stream, &a.counts)) return rc;
    HIP_TRY(hrt_launch_winding(a, r->winding_count.on, r->stream));
    return RT_OK;
}

// The moments on the host (rt_winding.hpp host_moments): pure CPU, no device.
int rt_host_tree_moments(const void* tris64, uint32_t n_tris, const void* hnodes, size_t node_slots, const uint32_t* order,
                         size_t n_order, uint32_t root_word, const float root[4], void* moments_out, size_t moment_cap) {
    const HostTree H("rt_host_tree_moments", false, tris64, n_tris, hnodes, node_slots, order, n_order, root_word, root);
    if (H.rc) return H.rc;
    if (node_slots == 0) return RT_OK;  // a tree without nodes has no records
    if (moment_cap < node_slots) return fail(RT_ERR_ARG, "rt_host_tree_moments: moment_cap is below node_slots");
    if (!moments_out) return fail(RT_ERR_ARG, "rt_host_tree_moments: null output");
    hrt_winding::Tree T{};
    H.fields(T);
    std::vector<float> rec(hrt_winding::REC_FLOATS * node_slots);
    if (!hrt_winding::host_moments(T, node_slots, n_order, rec.data()))
        return fail(RT_ERR_ARG, "rt_host_tree_moments: the nodes are not a tree over order and the triangles");
    std::memcpy(moments_out, rec.data(), rec.size() * sizeof(float));
    return RT_OK;
}

// The query on the host (rt_winding.hpp host_winding): pure CPU, no device; the bytes the device writes for that tree.
int rt_host_winding_numbers(const void* tris64, uint32_t n_tris, const void* hnodes, size_t node_slots, const uint32_t* order,
                            size_t n_order, uint32_t root_word, const float root[4], const float* points, uint32_t n,
                            float beta, float* w_out) {
    if (!hrt_winding::beta_ok(beta))
        return fail(RT_ERR_ARG, "rt_host_winding_numbers: beta must be 0 (the default 2.0) or at least 1 (+inf: no dipoles)");
    if (n && (!points || !w_out)) return fail(RT_ERR_ARG, "rt_host_winding_numbers: null points or w_out");
    const HostTree H("rt_host_winding_numbers", false, tris64, n_tris, hnodes, node_slots, order, n_order, root_word, root);
    if (H.rc) return H.rc;
    hrt_winding::Tree T{};
    H.fields(T);
    std::vector<float> rec(hrt_winding::REC_FLOATS * std::max<size_t>(node_slots, 1));
    if (node_slots && !hrt_winding::host_moments(T, node_slots, n_order, rec.data()))
        return fail(RT_ERR_ARG, "rt_host_winding_numbers: the nodes are not a tree over order and the triangles");
    T.moments = rec.data();
    hrt_winding::host_winding(T, points, n, beta, w_out);
    return RT_OK;
}

int rt_testing_winding_atan2(const float* y, const float* x, uint32_t n, float* out) {
    if (n && (!y || !x || !out)) return fail(RT_ERR_ARG, "rt_testing_winding_atan2: null");
    for (uint32_t i = 0; i < n; i++) out[i] = hrt_winding::atan2_f32(y[i], x[i]);
    return RT_OK;
}

int rt_testing_get_tree_moments(rt_renderer* r, void* moments_out, size_t moment_cap, size_t* count) {
    if (!r || !count) return fail(RT_ERR_ARG, "rt_testing_get_tree_moments: null");
    if (int rc = need_tri_tree(r, "rt_testing_get_tree_moments")) return rc;
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (int rc = upload_tri_tree(r)) return rc;  // (a host tree not built yet)
    if (int rc = ensure_moments(r)) return rc;
    const size_t slots = (r->tri_tree.root_word & hrt_winding::LEAF_BIT) != 0u ? 0u : r->tb_n_nodes;
    *count = slots;
    if (moment_cap == 0) return RT_OK;
    if (moment_cap < slots) return fail(RT_ERR_ARG, "rt_testing_get_tree_moments: moment_cap is too small");
    if (slots && !moments_out) return fail(RT_ERR_ARG, "rt_testing_get_tree_moments: null output");
    HIP_TRY(hipStreamSynchronize(r->stream));
    if (slots) HIP_TRY(hipMemcpy(moments_out, r->tb_moments.ptr, slots * 64u, hipMemcpyDeviceToHost));
    return RT_OK;
}

// ---- multi-hit ray queries (include/hrt.h; rt_multihit.hip k_cast_rays_multi, rt_multihit.hpp the function) ----
int rt_cast_rays_multi(rt_renderer* r, const void* origins_dev, const void* dirs_dev, const void* tmax_dev, const void* after_dev,
                       uint32_t n, uint32_t k, void* hits_dev, void* counts_dev) {
    if (!r) return fail(RT_ERR_ARG, "rt_cast_rays_multi: null");
    if (k > RT_MULTI_HIT_MAX_K) return fail(RT_ERR_ARG, "rt_cast_rays_multi: k exceeds RT_MULTI_HIT_MAX_K");
    if (n == 0) return RT_OK;
    if (k == 0 && !counts_dev) return fail(RT_ERR_ARG, "rt_cast_rays_multi: k = 0 needs counts");
    if (k > 0 && !hits_dev) return fail(RT_ERR_ARG, "rt_cast_rays_multi: k > 0 needs hits");
    if (!origins_dev || !dirs_dev) return fail(RT_ERR_ARG, "rt_cast_rays_multi: null buffer");
    if (misaligned(16, {hits_dev}) || misaligned(4, {origins_dev, dirs_dev, tmax_dev, after_dev, counts_dev}))
        return fail(RT_ERR_ARG, "rt_cast_rays_multi: hits must be 16-byte aligned, every other buffer 4-byte aligned");
    static_assert(sizeof(rt_multi_hit) == 16, "rt_multi_hit: one 16-byte store per record (k_cast_rays_multi)");
    QueryScope q(r, "rt_cast_rays_multi");
    if (q.rc) return q.rc;
    hrt_multihit::Launch a{};
    tree_fields(a.tree, q.P);
    a.origins = (const float*)origins_dev;
    a.dirs = (const float*)dirs_dev;
    a.tmax = (const float*)tmax_dev;
    a.after = (const hrt_multihit::Hit*)after_dev;
    a.hits = hits_dev;
    a.counts = (uint32_t*)counts_dev;
    a.n = n;
    a.k = k;
    if (int rc = r->multihit_count.arm(4, r->stream, &a.stats)) return rc;
    HIP_TRY(hrt_launch_multihit(a, r->multihit_count.on, r->stream));
    return RT_OK;
}

// The query on the host (rt_multihit.hpp host_multi): pure CPU, no device; the bytes the device writes for that tree.
int rt_host_cast_rays_multi(const void* tris64, uint32_t n_tris, const void* hnodes, size_t node_slots, const uint32_t* order,
                            size_t n_order, uint32_t root_word, const float root[4], const float* origins, const float* dirs,
                            const float* tmax, const void* after16, uint32_t n, uint32_t k, void* hits16, uint32_t* counts) {
    const char* const who = "rt_host_cast_rays_multi";
    if (k > RT_MULTI_HIT_MAX_K) return fail(RT_ERR_ARG, std::string(who) + ": k exceeds RT_MULTI_HIT_MAX_K");
    if (k == 0 && !counts) return fail(RT_ERR_ARG, std::string(who) + ": k = 0 needs counts");
    if (n && (!origins || !dirs || (k && !hits16))) return fail(RT_ERR_ARG, std::string(who) + ": null rays or hits");
    const HostTree H(who, true, tris64, n_tris, hnodes, node_slots, order, n_order, root_word, root);
    if (H.rc) return H.rc;
    hrt_multihit::Tree T{};
    H.fields(T);
    T.flat = node_slots ? 0u : 1u;
    if (node_slots && !hrt_multihit::host_tree_ok(T, node_slots, H.ord.size()))
        return fail(RT_ERR_ARG, std::string(who) + ": the nodes are not a tree over order and the triangles");
    std::vector<hrt_multihit::Hit> after, out((size_t)n * k);
    if (after16 && n) {
        after.resize(n);
        std::memcpy(after.data(), after16, (size_t)n * sizeof(hrt_multihit::Hit));
    }
    hrt_multihit::host_multi(T, origins, dirs, tmax, after16 ? after.data() : nullptr, n, k, out.data(), counts);
    if (!out.empty()) std::memcpy(hits16, out.data(), out.size() * sizeof(hrt_multihit::Hit));
    return RT_OK;
}

// ---- volume queries (include/hrt.h; rt_overlap.hip k_overlap, rt_overlap.hpp the function) ----
int rt_overlap_volumes(rt_renderer* r, uint32_t kind, const void* volumes_dev, const void* after_dev, uint32_t n, uint32_t k,
                       void* hits_dev, void* counts_dev) {
    if (!r) return fail(RT_ERR_ARG, "rt_overlap_volumes: null");
    if (k > RT_OVERLAP_MAX_K) return fail(RT_ERR_ARG, "rt_overlap_volumes: k exceeds RT_OVERLAP_MAX_K");
    if (kind != RT_VOLUME_BOX && kind != RT_VOLUME_BALL) return fail(RT_ERR_ARG, "rt_overlap_volumes: unknown kind");
    if (n == 0) return RT_OK;
    if (k == 0 && !counts_dev) return fail(RT_ERR_ARG, "rt_overlap_volumes: k = 0 needs counts");
    if (k > 0 && !hits_dev) return fail(RT_ERR_ARG, "rt_overlap_volumes: k > 0 needs hits");
    if (!volumes_dev) return fail(RT_ERR_ARG, "rt_overlap_volumes: null buffer");
    if (misaligned(16, {hits_dev}) || misaligned(4, {volumes_dev, after_dev, counts_dev}))
        return fail(RT_ERR_ARG, "rt_overlap_volumes: hits must be 16-byte aligned, every other buffer 4-byte aligned");
    static_assert(sizeof(rt_overlap_hit) == 16, "rt_overlap_hit: one 16-byte store per record (k_overlap)");
    QueryScope q(r, "rt_overlap_volumes");
    if (q.rc) return q.rc;
    hrt_overlap::Launch a{};
    tree_fields(a.tree, q.P);
    a.volumes = (const float*)volumes_dev;
    a.after = (const hrt_overlap::Hit*)after_dev;
    a.hits = hits_dev;
    a.counts = (uint32_t*)counts_dev;
    a.n = n;
    a.k = k;
    a.kind = kind;
    if (int rc = r->overlap_count.arm(4, r->stream, &a.stats)) return rc;
    HIP_TRY(hrt_launch_overlap(a, r->overlap_count.on, r->stream));
    return RT_OK;
}

// The query on the host (rt_overlap.hpp host_overlap): pure CPU, no device; the bytes the device writes for that tree.
int rt_host_overlap_volumes(const void* tris64, uint32_t n_tris, const void* hnodes, size_t node_slots, const uint32_t* order,
                            size_t n_order, uint32_t root_word, const float root[4], uint32_t kind, const float* volumes,
                            const void* after16, uint32_t n, uint32_t k, void* hits16, uint32_t* counts) {
    const char* const who = "rt_host_overlap_volumes";
    if (k > RT_OVERLAP_MAX_K) return fail(RT_ERR_ARG, std::string(who) + ": k exceeds RT_OVERLAP_MAX_K");
    if (kind != RT_VOLUME_BOX && kind != RT_VOLUME_BALL) return fail(RT_ERR_ARG, std::string(who) + ": unknown kind");
    if (n && k == 0 && !counts) return fail(RT_ERR_ARG, std::string(who) + ": k = 0 needs counts");
    if (n && (!volumes || (k && !hits16))) return fail(RT_ERR_ARG, std::string(who) + ": null volumes or hits");
    const HostTree H(who, true, tris64, n_tris, hnodes, node_slots, order, n_order, root_word, root);
    if (H.rc) return H.rc;
    hrt_overlap::Tree T{};
    H.fields(T);
    T.flat = node_slots ? 0u : 1u;
    if (node_slots && !hrt_multihit::host_tree_ok(T, node_slots, H.ord.size()))
        return fail(RT_ERR_ARG, std::string(who) + ": the nodes are not a tree over order and the triangles");
    std::vector<hrt_overlap::Hit> after, out((size_t)n * k);
    if (after16 && n) {
        after.resize(n);
        std::memcpy(after.data(), after16, (size_t)n * sizeof(hrt_overlap::Hit));
    }
    hrt_overlap::host_overlap(T, kind, volumes, after16 ? after.data() : nullptr, n, k, out.data(), counts);
    if (!out.empty()) std::memcpy(hits16, out.data(), out.size() * sizeof(hrt_overlap::Hit));
    return RT_OK;
}

int rt_regroup_paths(rt_renderer* r, const rt_regroup* io, uint32_t n) {
    if (!r) return fail(RT_ERR_ARG, "rt_regroup_paths: null");
    if (n == 0) return RT_OK;
    if (!io) return fail(RT_ERR_ARG, "rt_regroup_paths: null io");
    if (io->mode != RT_REGROUP_CELL_OCTANT && io->mode != RT_REGROUP_KEYS)
        return fail(RT_ERR_ARG, "rt_regroup_paths: unknown mode");
    if (io->reserved != 0) return fail(RT_ERR_ARG, "rt_regroup_paths: reserved must be 0");
    if (!io->index_out_dev) return fail(RT_ERR_ARG, "rt_regroup_paths: null index_out");
    if (io->mode == RT_REGROUP_CELL_OCTANT && (!io->origins_dev || !io->dirs_dev))
        return fail(RT_ERR_ARG, "rt_regroup_paths: mode 1 needs origins and dirs");
    if (io->mode == RT_REGROUP_KEYS && !io->keys_dev) return fail(RT_ERR_ARG, "rt_regroup_paths: mode 2 needs keys");
    if (n > RT_REGROUP_MAX_ENTRIES) return fail(RT_ERR_ARG, "rt_regroup_paths: more than RT_REGROUP_MAX_ENTRIES entries");
    if (!io->index_in_dev && n > io->paths) return fail(RT_ERR_ARG, "rt_regroup_paths: n exceeds paths without index_in");
    const bool cell = io->mode == RT_REGROUP_CELL_OCTANT;  // (a buffer the mode does not read is not looked at)
    if ((cell ? misaligned(4, {io->origins_dev, io->dirs_dev}) : misaligned(4, {io->keys_dev})) ||
        misaligned(4, {io->index_in_dev, io->count_in_dev, io->index_out_dev, io->keys_out_dev}))
        return fail(RT_ERR_ARG, "rt_regroup_paths: every buffer must be 4-byte aligned");
    static_assert(sizeof(rt_regroup) == 96, "rt_regroup: seven pointers, two words, six floats, two words (hrt/_lib.py RtRegroup)");
    hrt_regroup::Launch a{};
    if (cell && !hrt_regroup::box_inverse(io->box_lo, io->box_hi, a.inv))
        return fail(RT_ERR_ARG, "rt_regroup_paths: every box extent must be finite and at least 2^-60");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    const size_t tiles = ((size_t)n + RT_REGROUP_TILE - 1u) / RT_REGROUP_TILE;
    int rc = ensure(r->regroup_entries, 4u * (size_t)n);
    if (!rc) rc = ensure(r->regroup_counts, 256u * tiles + hrt_regroup::TAIL_WORDS);
    if (rc) return rc;
    a.origins = cell ? (const float*)io->origins_dev : nullptr;
    a.dirs = cell ? (const float*)io->dirs_dev : nullptr;
    a.keys = cell ? nullptr : (const uint32_t*)io->keys_dev;
    a.index_in = (const uint32_t*)io->index_in_dev;
    a.count_in = (const uint32_t*)io->count_in_dev;
    a.index_out = (uint32_t*)io->index_out_dev;
    a.keys_out = (uint32_t*)io->keys_out_dev;
    a.paths = io->paths;
    a.mode = io->mode;
    for (int k = 0; k < 3; k++) a.lo[k] = cell ? io->box_lo[k] : 0.0f;
    a.entries = r->regroup_entries.ptr;
    a.counts = r->regroup_counts.ptr;
    HIP_TRY(hrt_launch_regroup(a, n, r->stream));
    return RT_OK;
}

int rt_host_regroup_keys(const float* origins, const float* dirs, uint32_t n, const float box_lo[3], const float box_hi[3],
                         uint32_t* keys_out) {
    if (!box_lo || !box_hi) return fail(RT_ERR_ARG, "rt_host_regroup_keys: null box");
    float inv[3];
    if (!hrt_regroup::box_inverse(box_lo, box_hi, inv))
        return fail(RT_ERR_ARG, "rt_host_regroup_keys: every box extent must be finite and at least 2^-60");
    if (n == 0) return RT_OK;
    if (!origins || !dirs || !keys_out) return fail(RT_ERR_ARG, "rt_host_regroup_keys: null buffer");
    for (uint32_t i = 0; i < n; i++)
        keys_out[i] = hrt_regroup::cell_octant_key(origins + 3u * (size_t)i, dirs + 3u * (size_t)i, box_lo, inv);
    return RT_OK;
}

int rt_primary_rays(rt_renderer* r, uint32_t time, void* origins_dev, void* dirs_dev, size_t n_rays) {
    if (!r) return fail(RT_ERR_ARG, "rt_primary_rays: null");
    if (!r->has_camera) return fail(RT_ERR_STATE, "rt_set_camera must be called before rt_primary_rays");
    if (n_rays != (size_t)r->local_rows() * r->width)
        return fail(RT_ERR_ARG, "rt_primary_rays: n_rays must be local_rows x width");
    if (n_rays == 0) return RT_OK;
    if (!origins_dev || !dirs_dev) return fail(RT_ERR_ARG, "rt_primary_rays: null buffer");
    if (misaligned(4, {origins_dev, dirs_dev}))
        return fail(RT_ERR_ARG, "rt_primary_rays: origins and directions must be 4-byte aligned");
    QueryScope q(r);
    if (q.rc) return q.rc;
    HIP_TRY(hrt_launch_primary_rays(r->mode, q.P, time, (float*)origins_dev, (float*)dirs_dev, nullptr, r->stream));
    return RT_OK;
}

int rt_primary_rng(rt_renderer* r, uint32_t time, void* rng_dev, size_t n_rays) {
    if (!r) return fail(RT_ERR_ARG, "rt_primary_rng: null");
    if (!r->has_camera) return fail(RT_ERR_STATE, "rt_set_camera must be called before rt_primary_rng");
    if (n_rays != (size_t)r->local_rows() * r->width)
        return fail(RT_ERR_ARG, "rt_primary_rng: n_rays must be local_rows x width");
    if (n_rays == 0) return RT_OK;
    if (!rng_dev) return fail(RT_ERR_ARG, "rt_primary_rng: null buffer");
    if (misaligned(4, {rng_dev})) return fail(RT_ERR_ARG, "rt_primary_rng: the states must be 4-byte aligned");
    QueryScope q(r);
    if (q.rc) return q.rc;
    HIP_TRY(hrt_launch_primary_rays(r->mode, q.P, time, nullptr, nullptr, (uint32_t*)rng_dev, r->stream));
    return RT_OK;
}

int rt_get_stream(const rt_renderer* r, void** hip_stream) {
    if (!r || !hip_stream) return fail(RT_ERR_ARG, "rt_get_stream: null");
    *hip_stream = (void*)r->stream;
    return RT_OK;
}

int rt_read_image(rt_renderer* r, float* out, size_t n_floats) {
    if (!r || !out) return fail(RT_ERR_ARG, "rt_read_image: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (n_floats != r->image_floats()) return fail(RT_ERR_ARG, "rt_read_image: size mismatch");
    HIP_TRY(hipMemcpyAsync(out, r->image.ptr, n_floats * sizeof(float), hipMemcpyDeviceToHost, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return finish_stats(r);
}

int rt_write_image(rt_renderer* r, const float* in, size_t n_floats) {
    if (!r || !in) return fail(RT_ERR_ARG, "rt_write_image: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (n_floats != r->image_floats()) return fail(RT_ERR_ARG, "rt_write_image: size mismatch");
    HIP_TRY(hipMemcpyAsync(r->image.ptr, in, n_floats * sizeof(float), hipMemcpyHostToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return RT_OK;
}

int rt_copy_image_to_device(rt_renderer* r, void* dst, size_t n_floats) {
    if (!r || !dst) return fail(RT_ERR_ARG, "rt_copy_image_to_device: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (n_floats != r->image_floats()) return fail(RT_ERR_ARG, "rt_copy_image_to_device: size mismatch");
    HIP_TRY(hipMemcpyAsync(dst, r->image.ptr, n_floats * sizeof(float), hipMemcpyDeviceToDevice, r->stream));
    HIP_TRY(hipStreamSynchronize(r->stream));
    return finish_stats(r);
}

int rt_reset_frame_count(rt_renderer* r) {
    if (!r) return fail(RT_ERR_ARG, "rt_reset_frame_count: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    r->frame_count = 0;
    return zero_image(r);
}

int rt_resize(rt_renderer* r, uint32_t width, uint32_t height) {
    if (!r) return fail(RT_ERR_ARG, "rt_resize: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    r->width = std::max<uint32_t>(1, width);  // renderer.rs:274-275
    r->height = std::max<uint32_t>(1, height);
    r->cost_learn = true;
    r->frame_count = 0;
    return zero_image(r);
}

int rt_synchronize(rt_renderer* r) {
    if (!r) return fail(RT_ERR_ARG, "rt_synchronize: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    HIP_TRY(hipStreamSynchronize(r->stream));
    return finish_stats(r);
}

int rt_release_scratch(rt_renderer* r) {
    if (!r) return fail(RT_ERR_ARG, "rt_release_scratch: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (r->timing_pending) {
        const int rc = finish_stats(r);  // the pending draws' counters, and their kernels done
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(r->stream));
    r->samples.release();
    r->samples2.release();
    r->ring.release();
    r->ring_ctl.release();
    r->regroup_entries.release();
    r->regroup_counts.release();
    // rt_set_triangles_device's scratch and staging (the geometry before the last build), not the tree in use (tb_parent
    // is the tree's: a refit after this call allocates staging, arrivals and boxes again)
    r->lb_tris.release();
    r->lb_geo.release();
    r->lb_mats.release();
    r->lb_hnodes.release();
    r->lb_order.release();
    r->lb_keys.release();
    r->lb_parent.release();
    r->lb_arrivals.release();
    r->lb_boxes.release();
    r->lb_stat.release();
    r->tb_moments.release();  // (rt_winding_numbers makes the moments again)
    r->moments_dirty = true;
    return RT_OK;
}

int rt_get_stats(const rt_renderer* r, rt_stats* out) {
    if (!r || !out) return fail(RT_ERR_ARG, "rt_get_stats: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    int rc = finish_stats(const_cast<rt_renderer*>(r));
    if (rc) return rc;
    *out = r->stats;
    return RT_OK;
}

int rt_get_raw_counters(const rt_renderer* r, uint64_t* out, int n) {
    if (!r || !out || n < 0) return fail(RT_ERR_ARG, "rt_get_raw_counters: bad argument");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    int rc = finish_stats(const_cast<rt_renderer*>(r));
    if (rc) return rc;
    for (int i = 0; i < n; i++) out[i] = i < RT_RAW_COUNTERS ? r->raw_counters[i] : 0;
    return RT_OK;
}

int rt_get_wave_trace(rt_renderer* r, uint64_t* out, size_t n_words) {
    if (!r || !out) return fail(RT_ERR_ARG, "rt_get_wave_trace: null");
    DeviceScope ds(r->device);
    if (ds.rc) return ds.rc;
    if (n_words > r->wave_trace_words) return fail(RT_ERR_ARG, "rt_get_wave_trace: more words than recorded");
    if (n_words) HIP_TRY(hipMemcpy(out, r->wave_trace.ptr, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    return RT_OK;
}

int rt_get_device(const rt_renderer* r, int32_t* ordinal, int32_t pci[3]) {
    if (!r || !ordinal || !pci) return fail(RT_ERR_ARG, "rt_get_device: null");
    int v[3] = {0, 0, 0};
    HIP_TRY(hipDeviceGetAttribute(&v[0], hipDeviceAttributePciDomainId, r->device));
    HIP_TRY(hipDeviceGetAttribute(&v[1], hipDeviceAttributePciBusId, r->device));
    HIP_TRY(hipDeviceGetAttribute(&v[2], hipDeviceAttributePciDeviceId, r->device));
    *ordinal = r->device;
    for (int k = 0; k < 3; k++) pci[k] = v[k];
    return RT_OK;
}

int rt_check_exact_math(uint64_t n, uint32_t seed, uint64_t mismatches[3]) {
    if (!mismatches) return fail(RT_ERR_ARG, "rt_check_exact_math: null");
    int dev = 0;
    int rc = check_device(&dev);
    if (rc) return rc;
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, 3 * sizeof(unsigned long long)));
    hipError_t e = hipMemset(d, 0, 3 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hrt_check_exact_math(n, seed, d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(mismatches, d, 3 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, std::string("rt_check_exact_math: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_check_uniform_guards(uint64_t n_waves, uint32_t seed, uint64_t out[RT_UGUARD_HELPERS * RT_UGUARD_WORDS]) {
    if (!out) return fail(RT_ERR_ARG, "rt_check_uniform_guards: null");
    if (n_waves == 0) return fail(RT_ERR_ARG, "rt_check_uniform_guards: no waves");
    int dev = 0;
    int rc = check_device(&dev);
    if (rc) return rc;
    constexpr size_t bytes = RT_UGUARD_HELPERS * RT_UGUARD_WORDS * sizeof(unsigned long long);
    unsigned long long* d = nullptr;
    HIP_TRY(hipMalloc((void**)&d, bytes));
    hipError_t e = hipMemset(d, 0, bytes);
    if (e == hipSuccess) e = hrt_check_uniform_guards(n_waves, seed, d, nullptr);
    if (e == hipSuccess) e = hipMemcpy(out, d, bytes, hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(RT_ERR_DEVICE, std::string("rt_check_uniform_guards: ") + hipGetErrorString(e));
    return RT_OK;
}

int rt_diagnostic_build(void) {
#ifdef HRT_STAMPS
    return 1;
#else
    return 0;
#endif
}

}  // extern "C"
