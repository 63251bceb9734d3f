// rsd_internal.h -- librsd private state shared by the host entry points and the launchers.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>
#include <vector>

#include "../../include/rsd.h"
#include "bvh_build.h"

struct rsd_device {
    int hip_device = 0;
    int cu_count = 0;
};

namespace rsd {
// Alpha-masked materials on the device (csrc/alpha_test.h); triUV == null: none uploaded
struct AlphaData {
    const float* triUV = nullptr;      // 6 floats per primitive (uv0, uv1, uv2)
    const uint32_t* triMat = nullptr;  // material per primitive
    const float4* materials = nullptr; // {threshold (float16-rounded), constant alpha, texture (bits), 0}
    const uint4* textures = nullptr;   // {width, height, mip count, first texel}
    const uint8_t* texels = nullptr;   // all mips of all textures, R8
    float spread = 0.0f;               // RAY_CONE_SPREAD of the SD pass (set per launch)
};
}  // namespace rsd

namespace rsd {
// Per-frame-size ray terms of the SD setup (ray_table_kernel), keyed by what they depend on
struct RayTabCache {
    int w = -1, h = -1, guard = 0;
    uint32_t jitter = 0;
    float jx = 0.0f, jy = 0.0f;
    float camW[3] = {0.0f, 0.0f, 0.0f};
    int device = -1;
    float* d = nullptr;
    size_t cap = 0;
    bool same(const RayTabCache& k) const {
        return w == k.w && h == k.h && guard == k.guard && jitter == k.jitter && jx == k.jx && jy == k.jy &&
               camW[0] == k.camW[0] && camW[1] == k.camW[1] && camW[2] == k.camW[2] && device == k.device;
    }
    void setKey(const RayTabCache& k) {
        w = k.w; h = k.h; guard = k.guard; jitter = k.jitter; jx = k.jx; jy = k.jy;
        camW[0] = k.camW[0]; camW[1] = k.camW[1]; camW[2] = k.camW[2]; device = k.device;
    }
};

// Mutable SD-trace state of one (scene, stream) pair.  Traces of one scene on DIFFERENT
// streams may run concurrently (frames in flight): each stream owns its queue control,
// live-ray / key workspace and ray table, so concurrent launches never share scratch.
struct SdWorkspace {
    hipStream_t stream = nullptr;
    uint32_t* qctl = nullptr;      // live-ray queue control {count[32], head[32]} x 2 (double-buffered)
    uint32_t qctl_gen = 0;         // trace calls so far: buffer qctl_gen % 2 is zero and next in line
    bool qctl_dirty = true;        // reset both buffers before the next trace (first use, failed launch)
    void* queue = nullptr;         // live-ray records + K-key slots, grow-only
    size_t queue_cap = 0;          // bytes
    RayTabCache raytab;
    unsigned long long* counters = nullptr;  // 16 x u64 scratch of instrumented traces on this stream
    void* raster = nullptr;        // raster walk: slot map, tile records, 64-bit key lists (grow-only)
    size_t raster_cap = 0;         // bytes
};
void release_sd_workspaces(rsd_scene* s);

// What a dynamic scene (rsd_scene_upload_dynamic) keeps on the device for a refit (csrc/bvh_refit.hip):
// pointers into rsd_scene.d_dyn, one allocation
struct DynamicData {
    uint32_t* indices = nullptr;  // uint32[3 * triangle_count]
    float* positions = nullptr;   // float3[vertex_count]: the scene's copy, what the records were last written from
    uint32_t* parent = nullptr;   // per wide node: parent node << 2 | slot (the root: 0xffffffff)
    uint32_t* inner = nullptr;    // per wide node: its count of inner children
    uint32_t* arrive = nullptr;   // per wide node: inner children arrived in this refit (zero between refits)
    uint32_t* tight = nullptr;    // per wide node: its tight box as keys, lo[3] hi[3] (bvh_refit.h)
    // motion tracking (rsd_scene_track_motion): float3[vertex_count], the positions at the last
    // rsd_scene_motion_begin_frame; an allocation of its own (rsd_scene.motion_bytes), null when not tracked
    float* prev_positions = nullptr;
};
// The layout of rsd_scene.d_dyn for nt triangles, nv vertices and nn wide nodes: byte offsets of DynamicData's
// arrays, each 256-byte aligned.  The per-node tables follow the per-scene ones, so a rebuilt tree
// (rsd_scene_rebuild_bvh) keeps the order with another node count.
struct DynLayout {
    size_t indices, positions, parent, inner, arrive, tight, total;
};
inline DynLayout dyn_layout(uint32_t nt, uint32_t nv, uint32_t nn) {
    auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
    DynLayout l;
    l.indices = 0;
    l.positions = al(12 * (size_t)nt);
    l.parent = l.positions + al(12 * (size_t)nv);
    l.inner = l.parent + al(4 * (size_t)nn);
    l.arrive = l.inner + al(4 * (size_t)nn);
    l.tight = l.arrive + al(4 * (size_t)nn);
    l.total = l.tight + al(24 * (size_t)nn);
    return l;
}

// The rig of a dynamic scene (rsd_scene_attach_rig, csrc/skinning.hip): pointers into rsd_scene.d_rig, one
// allocation.  Every id in it was checked on the host at attach.
struct RigData {
    uint32_t count = 0, matrix_count = 0;
    uint32_t* vertex_ids = nullptr;  // uint32[count]
    uint32_t* matrix_ids = nullptr;  // uint32[count][4], 16-byte aligned
    float* weights = nullptr;        // float[count][4], 16-byte aligned
    float* rest = nullptr;           // float3[count]: what the matrices act on
    float* matrices = nullptr;       // float[matrix_count][12]: where a pose from host memory is copied
};

// The morph table of a rig (rsd_scene_attach_morph, csrc/skinning.hip): pointers into rsd_scene.d_morph, one
// allocation.  Offsets and weight ids were checked on the host at attach.
struct MorphData {
    uint32_t count = 0, weight_count = 0, entry_count = 0;
    uint32_t* offsets = nullptr;  // uint32[count + 1]
    uint4* entries = nullptr;     // {weight id, delta x, delta y, delta z (float bits)} per entry, 16-byte aligned
    float* weights = nullptr;     // float[weight_count]: the weights of the last pose (zeros after attach)
};
}  // namespace rsd

struct rsd_scene {
    rsd_device* dev = nullptr;
    float4* d_nodes = nullptr;   // one allocation: 8 x float4 per wide node, then
    float4* d_tris = nullptr;    //   3 x float4 per triangle record (d_tris = d_nodes + tri_offset)
    uint32_t tri_offset = 0;     // in float4 units
    uint32_t triangle_count = 0;
    uint32_t node_count = 0;
    rsd::BvhStats stats;
    uint32_t build_threads = 0;  // host threads of the BVH build
    uint64_t device_bytes = 0;
    uint64_t bvh_bytes = 0;      // the d_nodes allocation (nodes + triangle records + pad)
    uint32_t* d_prim_rec = nullptr;  // primitive id -> triangle record index (raster walk's keys)
    std::vector<rsd::SdWorkspace*> sd_ws;  // one per stream that traced this scene (few: linear lookup)
    std::mutex ws_mutex;                   // sd_ws: host threads may trace one scene on their own streams
    void* d_alpha = nullptr;       // alpha data (rsd_scene_upload_alpha), one allocation
    rsd::AlphaData alpha;          // device pointers into d_alpha
    // segment entry grid (entry_grid.h): one allocation, hash slots (uint4) then entry items
    void* d_entry = nullptr;
    uint32_t entry_bits = 0, entry_probe = 0, entry_rmax = 0, entry_cells = 0;
    float entry_origin[3] = {0.0f, 0.0f, 0.0f}, entry_extent = 0.0f;
    uint64_t entry_items_off = 0;  // bytes from d_entry to the item array
    uint64_t entry_bytes = 0;      // the d_entry allocation
    double entry_build_ms = 0.0;
    uint32_t* d_rtao_table = nullptr;  // RTAO's sample table (rtao.hip), uploaded by the first rsd_rtao
    // dynamic scenes (rsd_scene_upload_dynamic): d_dyn == null for every other scene
    void* d_dyn = nullptr;
    rsd::DynamicData dyn;
    uint32_t vertex_count = 0;
    uint64_t dyn_bytes = 0;
    uint64_t updates = 0;        // rsd_scene_update_* calls enqueued so far
    uint64_t motion_bytes = 0;       // dyn.prev_positions' allocation
    uint64_t motion_snapshots = 0;   // copies rsd_scene_motion_begin_frame enqueued
    uint64_t motion_seen_updates = 0;  // `updates` at the last snapshot: equal = prev_positions holds the positions
    // an update moved geometry since the entry grid was built: traces pass no table (the root-start path)
    // until rsd_scene_rebuild_entry_grid
    bool entry_stale = false;
    // animated scenes (rsd_scene_attach_rig): d_rig == null without a rig
    void* d_rig = nullptr;
    rsd::RigData rig;
    uint64_t rig_bytes = 0;
    // morph targets of the rig (rsd_scene_attach_morph): d_morph == null without a table
    void* d_morph = nullptr;
    rsd::MorphData morph;
    uint64_t morph_bytes = 0;
    // rsd_scene_rebuild_bvh calls that succeeded, and the last one's time on the device
    uint64_t rebuilds = 0;
    double rebuild_ms = 0.0;
};

namespace rsd {
void set_error(const std::string& msg);
rsd_status hip_fail(hipError_t e, const char* what);
// The end of a launcher: the status of the launch just enqueued
inline rsd_status launch_status(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, what);
}

// The image passes (post.hip, temporal_peel.hip, ao_resolve.hip, hbao.hip) run one lane per pixel in 64 x 4
// workgroups, so every wave reads whole cache lines of a row: the grid over a w x h rectangle of `layers` slices
constexpr int kImageBlockW = 64, kImageBlockH = 4;
inline dim3 image_block() { return dim3(kImageBlockW, kImageBlockH); }
inline dim3 image_grid(uint32_t w, uint32_t h, uint32_t layers = 1) {
    return dim3((w + kImageBlockW - 1) / kImageBlockW, (h + kImageBlockH - 1) / kImageBlockH, layers);
}

// bvh_refit.hip: the launches of one update of a dynamic scene on `st` -- scatter `count` positions into the
// scene's copy; rewrite the records from that copy and refit every box
rsd_status refit_scatter_enqueue(rsd_scene* s, const uint32_t* d_ids, const float* d_positions, uint32_t count,
                                 hipStream_t st);
rsd_status refit_enqueue(rsd_scene* s, hipStream_t st);
// lbvh.hip: rsd_scene_rebuild_bvh on a dynamic scene -- waits for the device, builds the LBVH of the current
// positions (csrc/lbvh.h) into new allocations, swaps it into `s`, refits its boxes and frees the old tree
rsd_status lbvh_rebuild(rsd_scene* s);
// prev_positions <- positions of a scene that tracks motion, one launch on `st`
rsd_status motion_snapshot_enqueue(rsd_scene* s, hipStream_t st);
// skinning.hip: pose the rig's vertices into the scene's position copy from `d_matrices` (float[matrix_count][12]);
// with a morph table the same launch first adds the table's deltas by the scene's weight table
rsd_status pose_enqueue(rsd_scene* s, const float* d_matrices, hipStream_t st);

// The previous camera's terms of the motion-vector projection (post.hip motion_vector_kernel, gbuffer_motion.hip):
// U / |U|^2, V / |V|^2, W / |W|^2, evaluated in double and rounded once
inline void mvec_prev_axes(const rsd_camera& prev, float pU[3], float pV[3], float pW[3]) {
    auto dot3 = [](const float* p, const float* q) { return (double)p[0] * q[0] + (double)p[1] * q[1] + (double)p[2] * q[2]; };
    const double uu = dot3(prev.U, prev.U), vv = dot3(prev.V, prev.V), ww = dot3(prev.W, prev.W);
    for (int k = 0; k < 3; ++k) {
        pU[k] = (float)(prev.U[k] / uu);
        pV[k] = (float)(prev.V[k] / vv);
        pW[k] = (float)(prev.W[k] / ww);
    }
}

// sd_trace.hip (host code): the stratified coverage-mask tables of N samples on HIP device `dev` (indices [N + 1], look-up
// table [2^N]), uploaded once per (device, N) and never freed; shared by the SD trace and sd_raster.hip
rsd_status sd_coverage_lut(int dev, uint32_t N, const int32_t** idx, const uint32_t** lut);

// halo.hip: the sparse-halo steps with the band frame's options (csrc/band_frame.cpp).  ilv: interleaved
// triples {texel, rayMin, rayMax} (a peer's prefix is one contiguous transfer); the SD lists then index
// with stride 3 (their idx points at the triples).  row: a count row zeroed ([0, row_n)) with
// row[row_n] = extra in the launch that zeroes the region counts; zeroed: the counts are already zero
// (the previous frame's compaction cleared them through zero_row), so the compaction launch alone writes
// row[row_n] and clears zero_row[0, row_n].
rsd_status halo_compact_impl(const uint32_t* d_ray_min, const uint32_t* d_ray_max, uint32_t sd_w, uint32_t sd_h,
                             const rsd_halo_region* regions, uint32_t n_regions, bool ilv, int64_t* row,
                             uint32_t row_n, int64_t extra, hipStream_t s, bool zeroed = false,
                             int64_t* zero_row = nullptr);
// the band frame's count matrix (n int64) to host-visible memory dst[1..n], then dst[0] = seq (system-scope
// release): the host polls dst[0] instead of waiting on an event
rsd_status publish_counts(const int64_t* d_src, int64_t* dst_host_dev, uint32_t n, int64_t seq, hipStream_t s);
rsd_status halo_merge_impl(uint32_t* d_ray_min, uint32_t* d_ray_max, uint32_t sd_w, uint32_t sd_h,
                           const rsd_halo_list* lists, uint32_t n_lists, uint32_t ray_interval, bool ilv,
                           hipStream_t s);
rsd_status halo_sd_impl(bool gather, float* sd, uint32_t layers, uint32_t sd_w, uint32_t sd_h, uint32_t ch,
                        const rsd_halo_sd_list* lists, uint32_t n_lists, bool ilv, hipStream_t s, const char* who);
}  // namespace rsd

#define RSD_HIP(call)                                                   \
    do {                                                                \
        hipError_t e_ = (call);                                         \
        if (e_ != hipSuccess) return rsd::hip_fail(e_, #call);          \
    } while (0)
