// bvh_refit.hip -- dynamic scenes: rewrite the triangle records from moved vertices and refit the boxes of
// the existing 4-wide tree on the GPU, in stream order (rsd_scene_update_positions / _subset).
//
// Also here: motion_snapshot_kernel, the copy of the positions into the previous positions of a scene that
// tracks motion (rsd_scene_motion_begin_frame).
//
// Two launches.  refit_records_kernel: one lane per triangle record gathers its three vertices through the
// index buffer and stores the nine position words; the prim / flags / pad words are never written.
// refit_boxes_kernel: one launch, bottom-up.  One lane per wide node computes the boxes of its LEAF children
// from the new records and stores those slots.  A node without inner children then climbs: it stores its
// tight box, stores the padded box into its parent's slot, publishes, and adds one to the parent's arrival
// counter; only the lane whose add completes the parent's count of inner children goes on with the parent
// (it recomputes the parent's leaf boxes in registers and reads the inner children's tight boxes), every
// other lane exits.  No lane ever waits for another, so the launch cannot deadlock whatever the placement
// or the occupancy, and the climb ends because a parent's index is below its children's.  The last arriver
// resets the counter, so the next update needs no memset.
//
// Box rule and its arithmetic: bvh_refit.h (integer keys and bit steps only; this file is also compiled
// without the fast-numerics flags, which the Makefile gives to *_fast.hip alone).
//
// Visibility across CUs (gfx950: a CU's vector L1 is never refreshed by another CU's stores, and the
// per-XCD L2s are not coherent with each other).  The only words one workgroup writes and another reads
// in this launch are the tight boxes.  The hand-off is the memory model's release / acquire pair at agent
// scope around the counter: the arriving lane stores its tight box with plain stores, runs
// fence(release, agent) -- which writes its XCD's dirty L2 lines back -- and then adds to the counter with
// an agent-scope atomic; the lane that finds the count complete runs fence(acquire, agent) -- which
// invalidates its CU's L1 -- before its first load of a child's tight box.  This is the architecturally
// guaranteed form; bypassing L1 with write-through stores and sc1 loads instead was not chosen because it
// is only an observed behaviour and every load of the handed-off words would have to be such a load.  An
// explicit s_waitcnt vmcnt(0) follows the release fence: the compiler may drop the fence's own wait when it
// believes the wave's vector-memory counter is empty, and the atomic must not overtake the write-back.
// The slot boxes a climbing lane stores into its parent are read by later launches only (a kernel boundary
// orders them), and the counters are touched by atomics alone.
#include <hip/hip_runtime.h>

#include "bvh_refit.h"
#include "rsd_internal.h"

namespace rsd {
namespace {

constexpr int kRefitBlock = 256;

__global__ __launch_bounds__(kRefitBlock) void refit_scatter_kernel(uint32_t* __restrict__ pos, uint32_t nv,
                                                                    const uint32_t* __restrict__ ids,
                                                                    const uint32_t* __restrict__ src, uint32_t count) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t v = ids[i];
    if (v >= nv) return;  // an id outside the scene moves nothing
    for (int k = 0; k < 3; ++k) pos[3 * (size_t)v + k] = src[3 * (size_t)i + k];
}

// Motion tracking (rsd_scene_motion_begin_frame): dst[0, n) <- src[0, n) in dwords.  Lanes [0, nvec) move one
// 16-byte vector each (nvec = n / 4 when both buffers are 16-byte aligned, the launcher's decision, else 0), the
// lanes after them one dword each of the tail [4 nvec, n).  A kernel, not a copy call: it sits in stream
// order with the refit launches and shows by name in a kernel trace.
__global__ __launch_bounds__(kRefitBlock) void motion_snapshot_kernel(uint32_t* __restrict__ dst,
                                                                      const uint32_t* __restrict__ src, uint32_t n,
                                                                      uint32_t nvec) {
    const uint32_t i = blockIdx.x * kRefitBlock + threadIdx.x;
    if (i < nvec) {
        reinterpret_cast<uint4*>(dst)[i] = reinterpret_cast<const uint4*>(src)[i];
        return;
    }
    const uint32_t k = 4u * nvec + (i - nvec);  // nvec <= n / 4 < 2^30: no wrap
    if (k < n) dst[k] = src[k];
}

__global__ __launch_bounds__(kRefitBlock) void refit_records_kernel(uint32_t* __restrict__ recs, uint32_t nt,
                                                                    const uint32_t* __restrict__ ind,
                                                                    const uint32_t* __restrict__ pos, uint32_t nv) {
    const uint32_t r = blockIdx.x * kRefitBlock + threadIdx.x;
    if (r >= nt) return;
    uint32_t* rec = recs + 12 * (size_t)r;
    const uint32_t prim = rec[3];
    if (prim >= nt) return;
    for (int j = 0; j < 3; ++j) {
        const uint32_t v = ind[3 * (size_t)prim + j];
        if (v >= nv) continue;
        const uint32_t x = pos[3 * (size_t)v], y = pos[3 * (size_t)v + 1], z = pos[3 * (size_t)v + 2];
        rec[4 * j] = x;  // xyz only: word 3 of each float4 (prim, flags, 0) is never written
        rec[4 * j + 1] = y;
        rec[4 * j + 2] = z;
    }
}

// the tight box of wide node `nd`: its leaf children from the records, its inner children from `tight`
// (withInner) -- or the leaf children alone, storing their slots (storeLeaves)
template <bool withInner, bool storeLeaves>
__device__ inline RefitBox node_tight(uint32_t* nd, const uint32_t* recs, const uint32_t* tight) {
    RefitBox all;
    refit_box_clear(all);
    for (uint32_t i = 0; i < 4; ++i) {
        const uint32_t ref = nd[24 + i], cnt = nd[28 + i];
        RefitBox b;
        if (cnt) {
            refit_box_clear(b);
            refit_box_grow_records(b, recs + 12 * (size_t)ref, cnt);
            if (storeLeaves) refit_store_slot(nd, i, b);
        } else if (withInner && ref != kRefitEmptyRef) {
            for (int k = 0; k < 3; ++k) {
                b.lo[k] = tight[6 * (size_t)ref + k];
                b.hi[k] = tight[6 * (size_t)ref + 3 + k];
            }
        } else {
            continue;
        }
        refit_box_grow(all, b);
    }
    return all;
}

__global__ __launch_bounds__(kRefitBlock) void refit_boxes_kernel(uint32_t* __restrict__ nodes, uint32_t nn,
                                                                  const uint32_t* __restrict__ recs,
                                                                  const uint32_t* __restrict__ parent,
                                                                  const uint32_t* __restrict__ inner,
                                                                  uint32_t* arrive, uint32_t* tight) {
    const uint32_t n = blockIdx.x * kRefitBlock + threadIdx.x;
    if (n >= nn) return;
    RefitBox all = node_tight<false, true>(nodes + 32 * (size_t)n, recs, nullptr);
    if (inner[n] != 0) return;  // the last of its inner children to arrive finishes this node
    uint32_t cur = n;
    for (;;) {
        const uint32_t p = parent[cur];
        if (p == kRefitNoParent) return;  // the root: its own box is stored nowhere
        const uint32_t pn = p >> 2;
        if (pn >= cur) return;  // not a tree of the builder's (checked at upload): never climb in a cycle
        for (int k = 0; k < 3; ++k) {
            tight[6 * (size_t)cur + k] = all.lo[k];
            tight[6 * (size_t)cur + 3 + k] = all.hi[k];
        }
        refit_store_slot(nodes + 32 * (size_t)pn, p & 3u, all);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        const uint32_t before = __hip_atomic_fetch_add(&arrive[pn], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (before + 1u != inner[pn]) return;  // not the last: exit, never wait
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        __hip_atomic_store(&arrive[pn], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        all = node_tight<true, false>(nodes + 32 * (size_t)pn, recs, tight);
        cur = pn;
    }
}

}  // namespace

rsd_status refit_scatter_enqueue(rsd_scene* s, const uint32_t* d_ids, const float* d_positions, uint32_t count,
                                 hipStream_t st) {
    if (!count) return RSD_OK;
    hipLaunchKernelGGL(refit_scatter_kernel, dim3((count + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st,
                       reinterpret_cast<uint32_t*>(s->dyn.positions), s->vertex_count, d_ids,
                       reinterpret_cast<const uint32_t*>(d_positions), count);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "refit_scatter_kernel launch");
}

rsd_status motion_snapshot_enqueue(rsd_scene* s, hipStream_t st) {
    const uint64_t n64 = 3 * (uint64_t)s->vertex_count;
    if (!n64) return RSD_OK;
    if (n64 > 0xffffff00ull) {  // the lane count below, rounded up to blocks, stays in 32 bits
        set_error("rsd_scene_motion_begin_frame: too many vertices for one launch");
        return RSD_ERR_UNSUPPORTED;
    }
    const uint32_t n = (uint32_t)n64;
    uint32_t* dst = reinterpret_cast<uint32_t*>(s->dyn.prev_positions);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(s->dyn.positions);
    const bool aligned = ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) == 0;
    const uint32_t nvec = aligned ? n / 4u : 0u;
    const uint32_t lanes = nvec + (n - 4u * nvec);
    hipLaunchKernelGGL(motion_snapshot_kernel, dim3((lanes + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st,
                       dst, src, n, nvec);
    return launch_status("motion_snapshot_kernel launch");
}

rsd_status refit_enqueue(rsd_scene* s, hipStream_t st) {
    const uint32_t nt = s->triangle_count, nn = s->node_count;
    if (!nt || !nn) return RSD_OK;
    uint32_t* nodes = reinterpret_cast<uint32_t*>(s->d_nodes);
    uint32_t* recs = reinterpret_cast<uint32_t*>(s->d_tris);
    hipLaunchKernelGGL(refit_records_kernel, dim3((nt + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, recs,
                       nt, s->dyn.indices, reinterpret_cast<const uint32_t*>(s->dyn.positions), s->vertex_count);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e, "refit_records_kernel launch");
    hipLaunchKernelGGL(refit_boxes_kernel, dim3((nn + kRefitBlock - 1) / kRefitBlock), dim3(kRefitBlock), 0, st, nodes,
                       nn, recs, s->dyn.parent, s->dyn.inner, s->dyn.arrive, s->dyn.tight);
    e = hipGetLastError();
    return e == hipSuccess ? RSD_OK : hip_fail(e, "refit_boxes_kernel launch");
}

}  // namespace rsd
