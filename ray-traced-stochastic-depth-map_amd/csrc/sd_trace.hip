// sd_trace.hip -- the host side of the SD trace: the coverage-mask tables, the per-(scene, stream) workspaces, SDArgs
// filled from the plan (sd_plan.h) and the scene, the launch sequence through sd_launch.h, the counters read back, and
// the rsd_sd_trace* entry points.  It defines no kernel; it is compiled as HIP because SDArgs lives in sd_common.h,
// beside the device code that reads it.  (Overview: sd_common.h)
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "sd_launch.h"

using namespace rsd;

namespace {
// coverage-mask tables per (device, N), process-wide, never freed (kernels in flight on any
// stream may read them)
struct LutCache {
    int32_t* d_idx = nullptr;
    uint32_t* d_lut = nullptr;
};
constexpr int kLutDevices = 64;
LutCache g_lut[kLutDevices][17];
std::mutex g_lut_mutex;

// the SD-trace workspace of (scene, stream); created on the stream's first trace.  Host threads may trace
// one scene on their own streams (the band frame's rank threads): the list is locked; a workspace is only
// used by its stream's calls, which the caller orders
constexpr size_t kMaxWorkspaces = 64;
rsd_status sd_workspace(rsd_scene* scene, hipStream_t s, SdWorkspace** out) {
    std::lock_guard<std::mutex> lock(scene->ws_mutex);
    for (SdWorkspace* w : scene->sd_ws)
        if (w->stream == s) { *out = w; return RSD_OK; }
    if (scene->sd_ws.size() >= kMaxWorkspaces) {
        // a caller cycling through many transient streams: drain the device (no trace of this
        // scene can still be using a workspace) and start over instead of growing without bound
        RSD_HIP(hipDeviceSynchronize());
        release_sd_workspaces(scene);
    }
    SdWorkspace* w = new SdWorkspace();
    w->stream = s;
    hipError_t e = hipMalloc(&w->qctl, 2 * kQctlWords * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&w->counters, 32 * sizeof(unsigned long long));
    if (e != hipSuccess) {
        (void)hipFree(w->qctl);
        delete w;
        return hip_fail(e, "sd workspace");
    }
    scene->sd_ws.push_back(w);
    *out = w;
    return RSD_OK;
}
}  // namespace

rsd_status rsd::sd_coverage_lut(int dev, uint32_t N, const int32_t** idx, const uint32_t** lut) {
    if (dev < 0 || dev >= kLutDevices || N > 16) {
        set_error("rsd_sd_trace: device index >= 64 or N > 16");
        return RSD_ERR_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> lock(g_lut_mutex);
    LutCache& c = g_lut[dev][N];
    if (!c.d_lut) {
        // StochasticDepthMapRT.cpp:79-124 generateStratifiedLookupTable
        std::vector<int32_t> ind(N + 1);
        std::vector<uint32_t> tab(1u << N);
        auto binom = [](int n, int k) {
            std::vector<int> C(k + 1, 0);
            C[0] = 1;
            for (int i = 1; i <= n; i++)
                for (int j = std::min(i, k); j > 0; j--) C[j] = C[j] + C[j - 1];
            return C[k];
        };
        ind[0] = 0;
        for (uint32_t i = 1; i <= N; i++) ind[i] = binom((int)N, (int)i - 1) + ind[i - 1];
        std::vector<int32_t> cur(ind);
        tab[0] = 0;
        for (uint32_t i = 1; i < (1u << N); i++) {
            int pc = __builtin_popcount(i);
            tab[cur[pc]] = i;
            cur[pc]++;
        }
        int32_t* di = nullptr;
        uint32_t* dl = nullptr;
        RSD_HIP(hipMalloc(&di, sizeof(int32_t) * ind.size()));
        RSD_HIP(hipMalloc(&dl, sizeof(uint32_t) * tab.size()));
        RSD_HIP(hipMemcpy(di, ind.data(), sizeof(int32_t) * ind.size(), hipMemcpyHostToDevice));
        RSD_HIP(hipMemcpy(dl, tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice));
        c.d_idx = di;
        c.d_lut = dl;
    }
    *idx = c.d_idx;
    *lut = c.d_lut;
    return RSD_OK;
}

namespace {
// The SD trace of the 8-row tile rows t = start + k * step, k < n (rsd_sd_trace_band_ex: an
// interleaved band; rsd_sd_trace_rows: a contiguous range).
//
// What runs is decided by sd_plan (sd_plan.cpp, host only and tested on the CPU); this function allocates what the
// plan sized, fills SDArgs from the plan and the scene's device pointers, and launches.

// Grow-only device scratch: a request beyond the capacity drains the stream (its earlier traces may still use the
// old allocation), then frees and reallocates
template <class T>
rsd_status grow_scratch(T*& d, size_t& cap, size_t need, hipStream_t s) {
    if (cap >= need) return RSD_OK;
    RSD_HIP(hipStreamSynchronize(s));
    (void)hipFree(d);
    d = nullptr;
    cap = 0;
    RSD_HIP(hipMalloc(&d, need));
    cap = need;
    return RSD_OK;
}

// A scene without geometry: every texel keeps DEFAULT_DEPTH
rsd_status sd_trace_empty(const rsd_sd_params* p, uint32_t* d_ray_min, uint32_t* d_ray_max, float* d_sd_out,
                          uint32_t sd_w, uint32_t sd_h, bool consume, rsd_counters* counters, rsd_stream stream) {
    const uint32_t N = p->sample_count;
    const float def = p->normalize ? 1.0f : 3.40282347e+37f;
    const size_t n = (size_t)sd_w * sd_h * (N < 4 ? N : 4) * ((N + 3) / 4);
    std::vector<float> h(n, def);
    std::vector<uint16_t> h16(n, p->normalize ? (uint16_t)0x3c00u : (uint16_t)0x7c00u);  // 1.0 / +inf
    if (p->use_16bit)
        RSD_HIP(hipMemcpyAsync(d_sd_out, h16.data(), n * 2, hipMemcpyHostToDevice, (hipStream_t)stream));
    else
        RSD_HIP(hipMemcpyAsync(d_sd_out, h.data(), n * 4, hipMemcpyHostToDevice, (hipStream_t)stream));
    RSD_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (consume) {
        rsd_status cs = rsd_svao_clear_intervals(d_ray_min, d_ray_max, sd_w * sd_h, stream);
        if (cs != RSD_OK) return cs;
    }
    if (counters) { *counters = rsd_counters{}; counters->rays_dispatched = (uint64_t)sd_w * sd_h; }
    return RSD_OK;
}

// The kernels' arguments that do not point into a workspace: the call's, the scene's and the plan's
SDArgs sd_args(const rsd_scene* scene, const rsd_camera* cam, const rsd_sd_params* p, const float* d_linear_z,
               uint32_t z_w, uint32_t z_h, uint32_t* d_ray_min, uint32_t* d_ray_max, float* d_sd_out, uint32_t sd_w,
               uint32_t sd_h, uint32_t start, uint32_t step, uint32_t n, bool consume, const SdPlan& pl) {
    SDArgs a{};
    a.nodes = scene->d_nodes;
    a.tris = scene->d_tris;
    a.triOff = scene->tri_offset;
    a.cam = *cam;
    a.linearZ = d_linear_z;
    a.zW = (int)z_w;
    a.zH = (int)z_h;
    a.rayMin = d_ray_min;
    a.rayMax = d_ray_max;
    a.sd = d_sd_out;
    a.sdW = (int)sd_w;
    a.sdH = (int)sd_h;
    a.guard = p->guard_band;
    a.impl = p->implementation;
    a.maxCount = p->max_count;
    a.jitter = p->jitter;
    a.normalize = p->normalize;
    a.rayInterval = p->ray_interval;
    a.cull = p->cull_mode;
    a.alpha = p->alpha;
    a.partCap = pl.partCap;
    a.bandStart = (int)start;
    a.bandStep = (int)step;
    a.bandN = (int)n;
    a.poolSoft = pl.poolSoft;
    a.deadFast = pl.deadFast;
    a.consume = consume ? 1u : 0u;
    a.rayMinW = d_ray_min;
    a.rayMaxW = d_ray_max;
    a.alphaTest = p->alpha_test && scene->d_alpha ? 1u : 0u;
    a.alphaData = scene->alpha;
    a.alphaData.spread = rsd_ray_cone_spread(cam->focalLength, sd_h);  // default texture dims = SD map
    a.f16 = p->use_16bit ? 1u : 0u;
    a.primRec = scene->d_prim_rec;
    if (pl.walk == 4) {
        a.raster = 1u;
        a.keysK = pl.K;
        a.nTris = scene->triangle_count;
        a.tilesW = pl.tilesW;
        for (int k = 0; k < 3; ++k) {
            a.projU[k] = pl.projU[k];
            a.projV[k] = pl.projV[k];
            a.projW[k] = pl.projW[k];
            a.camWn[k] = pl.camWn[k];
        }
        a.wClip = pl.wClip;
    }
    a.lpt = pl.lpt;
    a.lptLen = pl.lptLen;
    a.spread = pl.spread;
    a.quadStack = pl.quadStack;
    a.qrange = pl.qrange;
    a.hybridRowBlocks = pl.hybridRowBlocks;
    a.liveBlocks = pl.liveBlocks;
    a.rowPrio = pl.rowPrio;
    a.prio = pl.prio;
    a.tileState = p->d_tile_state;
    a.tileSig = pl.tileSig;
    a.tileCount = pl.tileCount;
    a.entOn = pl.entOn;
    // a dynamic scene whose geometry moved since the grid was built passes no table: its cells' frontiers need
    // not cover the triangles that moved into them (rsd_scene_rebuild_entry_grid makes it current again)
    const void* const entry = scene->entry_stale ? nullptr : scene->d_entry;
    a.entSlots = static_cast<const uint4*>(entry);
    a.entItems = entry ? reinterpret_cast<const float4*>(static_cast<const char*>(entry) + scene->entry_items_off)
                       : nullptr;
    a.entBits = scene->entry_bits;
    a.entProbe = scene->entry_probe;
    a.entRmax = (int)scene->entry_rmax;
    for (int k = 0; k < 3; ++k) a.entOrigin[k] = scene->entry_origin[k];
    a.entExtent = scene->entry_extent;
    a.diag = pl.diag;
    return a;
}

// The counters of an instrumented trace (and its diagnostics: RSD_TRACE_PHASES, RSD_TRACE_RAYLOG)
rsd_status sd_read_counters(const SdWorkspace* ws, const SdPlan& pl, const SdKnobs& knobs, uint32_t* rayLog,
                            rsd_counters* counters, hipStream_t s) {
    unsigned long long h[32];
    RSD_HIP(hipMemcpyAsync(h, ws->counters, sizeof(h), hipMemcpyDeviceToHost, s));
    RSD_HIP(hipStreamSynchronize(s));
    counters->rays_dispatched = h[0];
    counters->rays_active = h[1];
    counters->nodes_visited = h[2];
    counters->tris_tested = h[3];
    counters->hits_delivered = h[4];
    counters->max_nodes_per_ray = h[5];
    counters->max_steps_per_ray = h[6];
    counters->sum_ray_clocks = h[7];
    counters->max_ray_clocks = h[8];
    counters->leaves_visited = h[9];
    // walk: the hybrid an uninstrumented trace of this call takes (the kernels a caller's timed traces ran);
    // walk_instrumented: the walk this instrumented launch ran (its step clocks), never the hybrid
    counters->walk = (uint64_t)pl.walkReported;
    counters->walk_instrumented = (uint64_t)pl.walk;
    counters->entry_lookups = h[19];
    counters->entry_items = h[20];
    // row walk (instrumented): per-step clock sums and the clock of the instrumented launch
    counters->step_fetch_clocks = h[16];
    counters->step_compute_clocks = h[17];
    counters->step_pool_clocks = h[18];
    counters->row_steps = h[14];
    counters->texels_clean = h[25];
    counters->shader_clock_mhz = h[22] ? (double)h[21] / ((double)h[22] * 0.01) : 0.0;  // 100 MHz realtime
    if (knobs.phases)
        std::fprintf(stderr, "[rsd] row walk phase clocks: fetch %llu step %llu resolve %llu steps %llu loops %llu"
                     " | step split: mem %llu compute %llu pool %llu | compute split: box+sort %llu"
                     " tri-tests %llu merge+push %llu\n",
                     h[11], h[12], h[13], h[14], h[15], h[16], h[17], h[18], h[23], h[24], h[17] - h[23] - h[24]);
    if (rayLog) {
        std::vector<uint32_t> lg(pl.rayLogBytes / 4);
        RSD_HIP(hipMemcpy(lg.data(), rayLog, pl.rayLogBytes, hipMemcpyDeviceToHost));
        (void)hipFree(rayLog);
        if (FILE* f = std::fopen(knobs.rayLog.c_str(), "wb")) {
            std::fwrite(lg.data(), 4, lg.size(), f);
            std::fclose(f);
        }
    }
    if (h[10]) {  // the pool bound was violated: results of this trace are not reliable
        set_error("rsd_sd_trace: traversal pool overflow (BVH deeper than the row walk supports)");
        return RSD_ERR_HIP;
    }
    return RSD_OK;
}

rsd_status sd_trace_impl(rsd_scene* scene, const rsd_camera* cam, const rsd_sd_params* p, const float* d_linear_z,
                         uint32_t z_w, uint32_t z_h, uint32_t* d_ray_min, uint32_t* d_ray_max, float* d_sd_out,
                         uint32_t sd_w, uint32_t sd_h, uint32_t start, uint32_t step, uint32_t n, uint32_t flags,
                         rsd_counters* counters, rsd_stream stream) {
    const SdKnobs knobs = sd_knobs_from_env();  // read per call: tests and A/B runs set them between traces
    SdPlanIn in;
    in.nullArg = !scene || !cam || !p || !d_linear_z || !d_sd_out;
    in.sdW = sd_w; in.sdH = sd_h; in.zW = z_w; in.zH = z_h;
    in.start = start; in.step = step; in.n = n;
    in.flags = flags;
    in.rayMin = d_ray_min != nullptr;
    in.rayMax = d_ray_max != nullptr;
    in.counters = counters != nullptr;
    if (p) in.params = *p;
    if (cam) in.cam = *cam;
    if (scene) {
        in.cuCount = scene->dev->cu_count;
        in.wideDepth = scene->stats.wide_depth;
        in.entryTable = scene->d_entry && !scene->entry_stale;
        in.primRec = scene->d_prim_rec != nullptr;
        in.alphaData = scene->d_alpha != nullptr;
        in.triangleCount = scene->triangle_count;
    }
    SdPlan pl;
    std::string err;
    const rsd_status planned = sd_plan(in, knobs, &pl, &err);
    if (planned != RSD_OK) {
        set_error(err);
        return planned;
    }
    if (pl.buildKey != sd_setup_build_key()) {
        set_error("rsd_sd_trace: sd_plan.cpp and sd_setup.hip were built with different RSD_SETUP_WAVES / RSD_CLASS_TILES / RSD_LIVE_WAVES");
        return RSD_ERR_UNSUPPORTED;
    }
    const bool consume = (flags & RSD_SD_CONSUME_INTERVALS) != 0u;
    if (pl.empty) return sd_trace_empty(p, d_ray_min, d_ray_max, d_sd_out, sd_w, sd_h, consume, counters, stream);
    SDArgs a = sd_args(scene, cam, p, d_linear_z, z_w, z_h, d_ray_min, d_ray_max, d_sd_out, sd_w, sd_h, start, step, n,
                       consume, pl);
    if (p->implementation == RSD_SD_COVERAGE_MASK) {
        rsd_status ls = sd_coverage_lut(scene->dev->hip_device, p->sample_count, &a.lutIdx, &a.lut);
        if (ls != RSD_OK) return ls;
    }
    hipStream_t s = (hipStream_t)stream;
    SdWorkspace* ws = nullptr;
    {
        rsd_status st = sd_workspace(scene, s, &ws);
        if (st != RSD_OK) return st;
    }
    {
        // per-frame-size ray terms (recomputed when the SD map size, guard band or jitter change)
        RayTabCache& rt = ws->raytab;
        const RayTabCache key{(int)sd_w, (int)sd_h, p->guard_band, p->jitter, cam->jitterX, cam->jitterY,
                              {cam->W[0], cam->W[1], cam->W[2]}, scene->dev->hip_device};
        const bool grows = rt.cap < pl.rayTabBytes;
        rsd_status st = grow_scratch(rt.d, rt.cap, pl.rayTabBytes, s);
        if (st != RSD_OK) return st;
        if (grows || !rt.same(key)) {
            const hipError_t te = launch_ray_table(rt.d, (int)sd_w, (int)sd_h, p->guard_band, p->jitter, *cam, s);
            if (te != hipSuccess) return hip_fail(te, "ray_table_kernel launch");
            rt.setKey(key);
        }
        a.rayTab = rt.d;
    }
    if (counters) {
        // per (scene, stream): concurrent instrumented traces on other streams keep their own
        RSD_HIP(hipMemsetAsync(ws->counters, 0, 32 * sizeof(unsigned long long), s));
        a.counters = ws->counters;
    }
    // the live-ray workspace, in the plan's sections
    {
        rsd_status st = grow_scratch(ws->queue, ws->queue_cap, pl.workspaceBytes, s);
        if (st != RSD_OK) return st;
    }
    char* const base = static_cast<char*>(ws->queue);
    float4* queue = reinterpret_cast<float4*>(base);
    uint2* keys = reinterpret_cast<uint2*>(base + pl.keysOff);
    if (pl.entBytes) a.entQ = reinterpret_cast<uint32_t*>(base + pl.entOff);
    if (pl.twoPass) {
        a.touchList = reinterpret_cast<uint32_t*>(base + pl.touchOff);
        a.touchCap = pl.touchCap;
    }
    if (pl.rayLogBytes) {
        RSD_HIP(hipMalloc(&a.rayLog, pl.rayLogBytes));
        RSD_HIP(hipMemsetAsync(a.rayLog, 0, pl.rayLogBytes, s));
    }
    // double-buffered queue control (sd_setup_kernel); both buffers are reset on first use and
    // after a failed launch sequence
    if (ws->qctl_dirty) {
        RSD_HIP(hipMemsetAsync(ws->qctl, 0, 2 * kQctlWords * sizeof(uint32_t), s));
        ws->qctl_dirty = false;
    }
    uint32_t* qctl = ws->qctl + (ws->qctl_gen & 1u) * kQctlWords;
    a.qctlNext = ws->qctl + ((ws->qctl_gen + 1u) & 1u) * kQctlWords;
    if (pl.walk == 4) {
        rsd_status st = grow_scratch(ws->raster, ws->raster_cap, pl.rasterBytes, s);
        if (st != RSD_OK) return st;
        char* const rbase = static_cast<char*>(ws->raster);
        a.keys64 = reinterpret_cast<unsigned long long*>(rbase);
        a.slotMap = reinterpret_cast<int32_t*>(rbase + pl.slotOff);
        a.tileRec = reinterpret_cast<float2*>(rbase + pl.tileRecOff);
        a.liveTiles = reinterpret_cast<uint32_t*>(rbase + pl.liveTilesOff);
    }
    if (pl.launch) {
        // the setup (one-pass, or classify + live), then the walk the plan chose
        const uint32_t N = p->sample_count;
        hipError_t e = launch_sd_setup(a, pl, N, queue, qctl, s);
        if (e == hipSuccess) switch (pl.walk) {
            case 1: case 2: e = launch_sd_walk_row(a, pl, N, queue, qctl, keys, s); break;
            case 4: e = launch_sd_walk_raster(a, pl, N, queue, qctl, keys, s); break;
            case 5: e = launch_sd_walk_wavefront(a, pl, N, queue, qctl, s); break;
            case 6: e = launch_sd_walk_hybrid(a, pl, N, queue, qctl, keys, s); break;
            default: e = launch_sd_walk_quad(a, pl, N, queue, qctl, s); break;  // 0, and 3: its traversal-order stream
        }
        if (e != hipSuccess) {
            ws->qctl_dirty = true;
            return hip_fail(e, "sd_trace_kernel launch");
        }
        ws->qctl_gen++;
    }
    return counters ? sd_read_counters(ws, pl, knobs, a.rayLog, counters, s) : RSD_OK;
}

}  // namespace

extern "C" rsd_status rsd_sd_trace_band_ex(rsd_scene* scene, const rsd_camera* cam, const rsd_sd_params* p,
                                           const float* d_linear_z, uint32_t z_w, uint32_t z_h, uint32_t* d_ray_min,
                                           uint32_t* d_ray_max, float* d_sd_out, uint32_t sd_w, uint32_t sd_h,
                                           uint32_t band_index, uint32_t band_count, uint32_t flags,
                                           rsd_counters* counters, rsd_stream stream) {
    if (band_count == 0 || band_index >= band_count) {
        set_error("rsd_sd_trace_band: band_index must be < band_count");
        return RSD_ERR_INVALID_ARG;
    }
    const uint32_t tiles = (sd_h + kTile - 1) / kTile;
    const uint32_t n = tiles > band_index ? (tiles - band_index + band_count - 1) / band_count : 0u;
    return sd_trace_impl(scene, cam, p, d_linear_z, z_w, z_h, d_ray_min, d_ray_max, d_sd_out, sd_w, sd_h, band_index,
                         band_count, n, flags, counters, stream);
}

extern "C" rsd_status rsd_sd_trace_rows(rsd_scene* scene, const rsd_camera* cam, const rsd_sd_params* p,
                                        const float* d_linear_z, uint32_t z_w, uint32_t z_h, uint32_t* d_ray_min,
                                        uint32_t* d_ray_max, float* d_sd_out, uint32_t sd_w, uint32_t sd_h,
                                        uint32_t row0, uint32_t row1, uint32_t flags, rsd_counters* counters,
                                        rsd_stream stream) {
    if (row0 > row1 || row1 > sd_h || row0 % kTile != 0u || (row1 % kTile != 0u && row1 != sd_h)) {
        set_error("rsd_sd_trace_rows: rows must satisfy row0 <= row1 <= sd_h, multiples of 8 (row1 may be sd_h)");
        return RSD_ERR_INVALID_ARG;
    }
    const uint32_t t0 = row0 / kTile, t1 = (row1 + kTile - 1) / kTile;
    return sd_trace_impl(scene, cam, p, d_linear_z, z_w, z_h, d_ray_min, d_ray_max, d_sd_out, sd_w, sd_h, t0, 1u,
                         t1 - t0, flags, counters, stream);
}

extern "C" rsd_status rsd_sd_trace_band(rsd_scene* scene, const rsd_camera* cam, const rsd_sd_params* p,
                                        const float* d_linear_z, uint32_t z_w, uint32_t z_h,
                                        const uint32_t* d_ray_min, const uint32_t* d_ray_max, float* d_sd_out,
                                        uint32_t sd_w, uint32_t sd_h, uint32_t band_index, uint32_t band_count,
                                        rsd_counters* counters, rsd_stream stream) {
    return rsd_sd_trace_band_ex(scene, cam, p, d_linear_z, z_w, z_h, const_cast<uint32_t*>(d_ray_min),
                                const_cast<uint32_t*>(d_ray_max), d_sd_out, sd_w, sd_h, band_index, band_count, 0u,
                                counters, stream);
}

extern "C" uint32_t rsd_sd_tile_state_count(uint32_t sd_w, uint32_t sd_h) {
    // per 8x8 tile a stamp word, then (ABI v8) per tile the two words of its 64-texel DEFAULT mask
    return 3u * ((sd_w + kTile - 1) / kTile) * ((sd_h + kTile - 1) / kTile);
}

extern "C" rsd_status rsd_sd_trace(rsd_scene* scene, const rsd_camera* cam, const rsd_sd_params* p,
                                   const float* d_linear_z, uint32_t z_w, uint32_t z_h, const uint32_t* d_ray_min,
                                   const uint32_t* d_ray_max, float* d_sd_out, uint32_t sd_w, uint32_t sd_h,
                                   rsd_counters* counters, rsd_stream stream) {
    return rsd_sd_trace_band(scene, cam, p, d_linear_z, z_w, z_h, d_ray_min, d_ray_max, d_sd_out, sd_w, sd_h, 0, 1,
                             counters, stream);
}

namespace rsd {
void release_sd_workspaces(rsd_scene* scene) {
    for (SdWorkspace* w : scene->sd_ws) {
        (void)hipFree(w->qctl);
        (void)hipFree(w->queue);
        (void)hipFree(w->raytab.d);
        (void)hipFree(w->counters);
        (void)hipFree(w->raster);
        delete w;
    }
    scene->sd_ws.clear();
}
}  // namespace rsd
