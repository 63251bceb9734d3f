// sd_plan.h -- the launch plan of one SD trace (host only: no HIP, no device pointers).
//
// sd_plan() takes the sizes, parameters and scene facts of one rsd_sd_trace* call and the RSD_TRACE_* /
// RSD_SETUP_* knobs, and decides everything sd_trace.hip then launches (through sd_launch.h): the walk, K, the LDS pool, the grids, the
// setup variant and the layout of the workspaces.  It is a pure function (tests/test_sd_plan.py checks it on the
// CPU), and this header holds the launch-geometry constants the plan and the kernels must agree on, each defined
// once.
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>

#include "../../include/rsd.h"
#include "entry_grid.h"

namespace rsd {

constexpr int kTile = 8;               // 8x8 texels per wave
constexpr uint32_t kQueueParts = 32;   // live-ray queue partitions (counter sharding)
constexpr int kBlock = kTile * kTile;  // 64 threads

// queue-control words of one trace: {count[32], head[32]} of the live-ray queue partitions, the
// raster walk's live-tile count, spare
constexpr int kQctlWords = 5 * (int)kQueueParts + 32;
constexpr int kQctlTouch = 4 * (int)kQueueParts + 32;  // two-pass setup: touched texels listed per partition
constexpr int kQctlHead2 = 3 * (int)kQueueParts + 32;  // hybrid walk: the row walk's own dequeue heads
constexpr int kQctlLiveTiles = 2 * (int)kQueueParts;
constexpr int kQctlShort = 2 * (int)kQueueParts + 32;  // lpt: short-ray counts (filled from the partition's end)
#ifndef RSD_SETUP_WAVES
#define RSD_SETUP_WAVES 4
#endif
constexpr int kSetupWaves = RSD_SETUP_WAVES;  // sd_setup_kernel: tiles (waves) per workgroup (A/B: RSD_SETUP_WAVES)
constexpr int kClassWaves = 4;   // sd_classify_kernel: waves per workgroup
#ifndef RSD_CLASS_TILES
#define RSD_CLASS_TILES 4
#endif
constexpr int kClassTiles = RSD_CLASS_TILES;  // sd_classify_kernel: 8x8 tiles per wave (their loads in one round trip)
constexpr int kLiveBlock = 256;  // sd_live_kernel: lanes per workgroup (4 waves)
#ifndef RSD_LIVE_WAVES
#define RSD_LIVE_WAVES 1  // sd_live_kernel: amdgpu_waves_per_eu (A/B)
#endif
// the three A/B macros above as one word: sd_plan.cpp records the values it was compiled with (SdPlan.buildKey), and
// a library whose sd_setup.hip was compiled with others (make variant DEFS=...) refuses to launch
constexpr uint32_t kPlanBuildKey = (uint32_t)RSD_SETUP_WAVES | (uint32_t)RSD_CLASS_TILES << 8 | (uint32_t)RSD_LIVE_WAVES << 16;

constexpr int kQuadRays = kBlock / 4;   // quad walks: rays per wave
// per-ray LDS stack of the quad walks, sized per scene at launch (dynamic LDS, SDArgs.quadStack): a
// depth-first 4-wide walk holds <= 3 pushed siblings per level below its start, plus the entry items it
// has not popped yet, so quad_stack_entries(wide depth) entries never overflow.  Sized to the tree, the
// stack of configs[1]-[4]'s trees (4-wide depth 15-18: 56-64 entries) takes 7-8 KB per wave instead of round 4's fixed 96
// entries (12 KB), and LDS no longer caps the persistent waves below their register limit (13 per CU).
constexpr uint32_t quad_stack_entries(uint32_t wideDepth) { return (3u * wideDepth + 7u + 7u) & ~7u; }
constexpr int kRasterBlock = 256;  // sd_raster_kernel: lanes (triangle records) per workgroup
constexpr int kPoolCap = 256;  // row walk: work items per ray (LDS: rays per wave x 256 x 8 B)

// The RSD_TRACE_* / RSD_SETUP_* environment knobs (A/B runs, diagnostics, tests that force a walk): read by
// sd_knobs_from_env() once per trace call.  The defaults below are those of an empty environment.
struct SdKnobs {
    enum Walk { kWalkAuto, kWalkQuad, kWalkFused, kWalkSplit, kWalkRaster };
    enum Hybrid { kHybridAuto, kHybridOff, kHybridAll };
    Walk walk = kWalkAuto;        // RSD_TRACE_WALK = quad | fused | split | raster
    Hybrid hybrid = kHybridAuto;  // RSD_TRACE_HYBRID = off | all
    bool hybrid16 = false;        // RSD_TRACE_HYBRID16 = on: the hybrid walk at K = 16 too
    uint32_t hybridRowWpc = 0;    // RSD_TRACE_HYBRID_ROWWPC: the hybrid's row blocks per CU (0: the default, 4)
    uint32_t wavesPerCu = 0;      // RSD_TRACE_WAVES_PER_CU: persistent blocks per CU (0: the walk's default)
    bool entry = true;            // RSD_TRACE_ENTRY = off: every ray walks from the root
    bool spec = true;             // RSD_TRACE_SPEC = off: the generic walks
    bool lpt = true;              // RSD_TRACE_LPT = off: no longest-first queue
    float lptLen = -0.1f;         // RSD_TRACE_LPT = a threshold (> 0 absolute, < 0 relative to TMin)
    bool pool256 = false;         // RSD_TRACE_POOL = 256: the row walk's large LDS pool
    bool prio = false;            // RSD_TRACE_PRIO = on: SDArgs.prio
    bool rowPrio = false;         // RSD_TRACE_ROWPRIO = on: SDArgs.rowPrio
    bool spread = false;          // RSD_TRACE_SPREAD = on: SDArgs.spread
    uint32_t qrange = 0;          // RSD_TRACE_QRANGE = long (1) | short (2): SDArgs.qrange (diagnostics)
    uint32_t diag = 0;            // RSD_SETUP_DIAG = skip (1) | nolive (2): SDArgs.diag (results wrong by design)
    int twoPass = 0;              // RSD_SETUP_TWOPASS = on (1) | off (-1)
    std::string rayLog;           // RSD_TRACE_RAYLOG: file of the instrumented walk's per-ray log
    bool phases = false;          // RSD_TRACE_PHASES: print the instrumented row walk's phase clocks
};
SdKnobs sd_knobs_from_env();

// What the decisions depend on, as plain values.
struct SdPlanIn {
    bool nullArg = false;  // a required pointer of the call is null (params is then all zero)
    uint32_t sdW = 0, sdH = 0, zW = 0, zH = 0;
    uint32_t start = 0, step = 1, n = 0;  // the 8-row tile rows start + k * step, k < n
    rsd_sd_params params{};               // d_tile_state is not looked at
    uint32_t flags = 0;                   // RSD_SD_CONSUME_INTERVALS | RSD_SD_THROUGHPUT
    bool rayMin = false, rayMax = false;  // the interval maps were given
    bool counters = false;                // an instrumented trace
    rsd_camera cam{};
    int cuCount = 0;
    uint32_t wideDepth = 0;      // rsd_scene.stats.wide_depth
    bool entryTable = false;     // the scene has an entry grid and it is current
    bool primRec = false;        // the scene has its primitive -> record map (raster walk)
    bool alphaData = false;      // the scene has alpha data
    uint32_t triangleCount = 0;
};

struct SdPlan {
    bool empty = false;   // a scene without triangles: every texel keeps DEFAULT_DEPTH, nothing else is decided
    bool launch = false;  // false: no tile row to trace (the workspaces are still sized)
    uint32_t buildKey = 0;
    // walk: 0 = quad (depth-first), 1 = row walk + in-kernel algorithm, 2 = split (row walk -> keys -> resolve
    // kernel), 3 = traversal-order any-hit stream, 4 = raster (triangles -> 64-bit key lists -> resolve kernel),
    // 5 = wavefront order, 6 = hybrid (row walk over the longest-first rays, quad walk over the rest)
    int walk = 0;          // the walk launched (counters.walk_instrumented)
    int walkReported = 0;  // counters.walk: the walk an uninstrumented trace of this call takes
    uint32_t K = 0, ROW = 0;
    bool split = false;  // one chunk of K keys decides every texel (the key section exists)
    bool spec = false;   // the specialised row / quad walk
    bool counters = false;
    int pool = 0, poolSoft = 0;
    uint32_t quadStack = 0;
    size_t ldsBytes = 0;  // dynamic LDS of the walk kernel
    uint32_t setupGrid[2] = {0, 0}, classGrid[2] = {0, 0}, liveBlocks = 0, rasterBlocks = 0;
    uint32_t persistentBlocks = 0, hybridRowBlocks = 0, rowPrio = 0, prio = 0;
    uint32_t lpt = 0;
    float lptLen = 0.0f;
    uint32_t spread = 0, qrange = 0, diag = 0;
    uint32_t entOn = 0, deadFast = 0;
    double cosLower = 0.0;
    bool twoPass = false;
    uint32_t touchCap = 0, partCap = 0;
    uint32_t tileSig = 0, tileCount = 0;
    // the workspace: sections in this order, byte offsets from its base (a section of 0 bytes is absent)
    size_t queueBytes = 0, keysOff = 0, keyBytes = 0, entOff = 0, entBytes = 0, touchOff = 0, touchBytes = 0;
    size_t workspaceBytes = 0;
    size_t rayLogBytes = 0;  // an allocation of its own (RSD_TRACE_RAYLOG)
    // the raster walk's workspace (walk 4 only)
    size_t keys64Bytes = 0, slotOff = 0, slotBytes = 0, tileRecOff = 0, tileRecBytes = 0, liveTilesOff = 0,
           liveTilesBytes = 0, rasterBytes = 0;
    // the raster walk's projection onto the SD texel grid (walk 4 only; SDArgs)
    float projU[3] = {0, 0, 0}, projV[3] = {0, 0, 0}, projW[3] = {0, 0, 0}, camWn[3] = {0, 0, 0}, wClip = 0.0f;
    int tilesW = 0;
    size_t rayTabBytes = 0;  // ray_table_kernel's table
};

// Validates the call and decides the launch.  Status and message (*err) are those rsd_sd_trace* reports.
rsd_status sd_plan(const SdPlanIn& in, const SdKnobs& knobs, SdPlan* plan, std::string* err);

}  // namespace rsd
