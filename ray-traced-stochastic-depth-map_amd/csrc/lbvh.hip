// lbvh.hip -- rsd_scene_rebuild_bvh: a new 4-wide tree over a dynamic scene's current positions, built on the
// GPU and swapped into the same rsd_scene.  The tree is defined in lbvh.h (shared with the host builder
// lbvh_host.cpp, whose bytes these launches reproduce); boxes come from the existing refit (bvh_refit.hip).
//
// Launches, in order, all on the null stream between two device waits:
//   scene_box_kernel   min / max keys of the referenced vertices: per-lane boxes, a wave reduction, then six
//                      integer atomics per wave (min / max of integers: the result does not depend on the order)
//   keys_kernel        one lane per triangle: its 64-bit key
//   rocprim radix sort of the keys (bits 0..61)
//   karras_kernel      one lane per internal binary node: range, split, and its children's parent words
//   depth_kernel       one lane per internal binary node: its depth up the parent chain; a node at an even depth
//                      with more than 4 triangles is a wide node and gets the sort key (wide depth, first position),
//                      every other node a key past all of those; counts the wide nodes and the deepest level
//   rocprim radix sort of (key, binary node) pairs: position w of the result is wide node w
//   -- the host reads the node count and the depth back and allocates the tree --
//   wide_index_kernel  one lane per wide node: binary node -> wide index
//   wide_kernel        one lane per wide node: ref / cnt of its slots, its inner children's parent words, its
//                      count of inner children
//   records_kernel     one lane per record: prim and flags words (flags from the primitive's old record) and the
//                      primitive -> record map
//   refit_enqueue      positions of the records and every box
// Every dependency between lanes is a kernel boundary: no lane waits for another inside a launch.  (rocprim's
// sort is the library's own code.)
//
// Bounds: every index a lane forms is checked against its array before use (karras positions lie in [0, nt) by
// lbvh_delta's range test; child ids and wide indices are compared with their counts).
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>

#include <algorithm>
#include <string>
#include <vector>

#include "bvh_traverse.h"
#include "lbvh.h"
#include "rsd_internal.h"

namespace rsd {
static_assert(kLbvhStackEntries == (uint32_t)kStackTotal, "lbvh.h's depth bound is derived from the walks' stack size");

namespace {

constexpr int kLbvhBlock = 256;
constexpr uint32_t kNotWideLevel = 63;  // the sort key's level of a binary node that is no wide node
constexpr uint32_t kWideKeyBits = 38;   // 32 bits of first position, 6 of level
// control words the host reads back
enum { kCtlWide = 0, kCtlLevel = 1, kCtlDepth = 2, kCtlLeaves = 3, kCtlWords = 4 };

__device__ inline uint32_t wave_min(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
        v = o < v ? o : v;
    }
    return v;
}
__device__ inline uint32_t wave_max(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t o = (uint32_t)__shfl_xor((int)v, m);
        v = o > v ? o : v;
    }
    return v;
}

__device__ inline uint32_t wave_sum(uint32_t v) {
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m);
    return v;
}

// box: lo[3] (preset to 0xffffffff) then hi[3] (preset to 0), as keys
__global__ __launch_bounds__(kLbvhBlock) void scene_box_kernel(const uint32_t* __restrict__ ind,
                                                               const uint32_t* __restrict__ pos, uint32_t nv,
                                                               uint32_t nt, uint32_t* box) {
    RefitBox b;
    refit_box_clear(b);
    const uint64_t n = 3ull * nt;
    for (uint64_t c = (uint64_t)blockIdx.x * kLbvhBlock + threadIdx.x; c < n; c += (uint64_t)gridDim.x * kLbvhBlock) {
        const uint32_t v = ind[c];
        if (v >= nv) continue;
        for (int k = 0; k < 3; ++k) {
            const uint32_t key = refit_key(pos[3 * (size_t)v + k]);
            b.lo[k] = key < b.lo[k] ? key : b.lo[k];
            b.hi[k] = key > b.hi[k] ? key : b.hi[k];
        }
    }
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = wave_min(b.lo[k]);
        b.hi[k] = wave_max(b.hi[k]);
    }
    if ((threadIdx.x & 63u) == 0u)
        for (int k = 0; k < 3; ++k) {
            atomicMin(&box[k], b.lo[k]);
            atomicMax(&box[3 + k], b.hi[k]);
        }
}

__global__ __launch_bounds__(kLbvhBlock) void keys_kernel(const uint32_t* __restrict__ ind,
                                                          const uint32_t* __restrict__ pos, uint32_t nv, uint32_t nt,
                                                          const uint32_t* __restrict__ box, uint64_t* __restrict__ keys) {
    const uint32_t t = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (t >= nt) return;
    RefitBox b;
    for (int k = 0; k < 3; ++k) {
        b.lo[k] = box[k];
        b.hi[k] = box[3 + k];
    }
    keys[t] = lbvh_key(t, ind, pos, nv, b);
}

// parent: preset to 0xffffffff (the root keeps it)
__global__ __launch_bounds__(kLbvhBlock) void karras_kernel(const uint64_t* __restrict__ keys, uint32_t nt,
                                                            uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                            uint32_t* __restrict__ split, uint32_t* __restrict__ parent) {
    const uint32_t i = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (nt < 2u || i >= nt - 1u) return;
    const LbvhNode n = lbvh_karras(keys, nt, i);
    first[i] = n.first;
    last[i] = n.last;
    split[i] = n.split;
    if (n.first != n.split && n.split < nt - 1u) parent[n.split] = i;
    if (n.split + 1u != n.last && n.split + 1u < nt - 1u) parent[n.split + 1u] = i;
}

__global__ __launch_bounds__(kLbvhBlock) void depth_kernel(uint32_t ni, const uint32_t* __restrict__ first,
                                                           const uint32_t* __restrict__ last,
                                                           const uint32_t* __restrict__ parent,
                                                           uint64_t* __restrict__ wkey, uint32_t* __restrict__ wval,
                                                           uint32_t* ctl) {
    const uint32_t i = blockIdx.x * kLbvhBlock + threadIdx.x;
    uint32_t depth = 0, below = 0, level = 0;
    bool wide = false;
    if (i < ni) {
        // distinct 64-bit keys: at most 63 ancestors; the bound also ends the walk on a table that is no tree
        for (uint32_t p = parent[i]; p < ni && depth < 64u; p = parent[p]) ++depth;
        wide = (depth & 1u) == 0u && last[i] - first[i] + 1u > kLbvhLeaf;
        wkey[i] = lbvh_wide_key(wide ? depth / 2u : kNotWideLevel, first[i]);
        wval[i] = i;
        below = depth + 1u;
        level = wide ? depth / 2u : 0u;
    }
    // one set of atomics per wave (every lane of the wave is here: no early return above)
    below = wave_max(below);
    level = wave_max(level);
    const uint32_t count = wave_sum(wide ? 1u : 0u);
    if ((threadIdx.x & 63u) == 0u) {
        atomicMax(&ctl[kCtlDepth], below);
        atomicMax(&ctl[kCtlLevel], level);
        if (count) atomicAdd(&ctl[kCtlWide], count);
    }
}

__global__ __launch_bounds__(kLbvhBlock) void wide_index_kernel(uint32_t nn, uint32_t ni,
                                                                const uint32_t* __restrict__ wval,
                                                                uint32_t* __restrict__ widx) {
    const uint32_t w = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (w >= nn) return;
    const uint32_t i = wval[w];
    if (i < ni) widx[i] = w;
}

// nodes: zeroed (empty slots keep zero boxes); parentOut / innerOut: the refit's tables of the new tree
__global__ __launch_bounds__(kLbvhBlock) void wide_kernel(uint32_t nn, uint32_t ni, const uint32_t* __restrict__ wval,
                                                          const uint32_t* __restrict__ widx,
                                                          const uint32_t* __restrict__ first,
                                                          const uint32_t* __restrict__ last,
                                                          const uint32_t* __restrict__ split, uint32_t* __restrict__ nodes,
                                                          uint32_t* __restrict__ parentOut, uint32_t* __restrict__ innerOut,
                                                          uint32_t* ctl) {
    const uint32_t w = blockIdx.x * kLbvhBlock + threadIdx.x;
    uint32_t leaves = 0;
    if (w < nn) {
        const uint32_t i = wval[w];
        uint32_t ref[4] = {kRefitEmptyRef, kRefitEmptyRef, kRefitEmptyRef, kRefitEmptyRef}, cnt[4] = {0u, 0u, 0u, 0u};
        uint32_t inner = 0;
        if (i < ni) {
            const LbvhSlots s = lbvh_slots(first, last, split, i);
            for (uint32_t k = 0; k < s.n; ++k) {
                const uint32_t size = s.b[k] - s.a[k] + 1u;
                if (size > kLbvhLeaf) {
                    const uint32_t c = s.id[k] < ni ? widx[s.id[k]] : kRefitEmptyRef;
                    if (c >= nn || c <= w) continue;  // never for a tree of the definition: leave the slot empty
                    ref[k] = c;
                    parentOut[c] = w << 2 | k;
                    ++inner;
                } else {
                    ref[k] = s.a[k];
                    cnt[k] = size;
                    ++leaves;
                }
            }
        }
        uint4* nd = reinterpret_cast<uint4*>(nodes + 32 * (size_t)w);
        nd[6] = make_uint4(ref[0], ref[1], ref[2], ref[3]);
        nd[7] = make_uint4(cnt[0], cnt[1], cnt[2], cnt[3]);
        innerOut[w] = inner;
        if (w == 0u) parentOut[0] = kRefitNoParent;
    }
    leaves = wave_sum(leaves);  // every lane of the wave is here
    if ((threadIdx.x & 63u) == 0u && leaves) atomicAdd(&ctl[kCtlLeaves], leaves);
}

__global__ __launch_bounds__(kLbvhBlock) void records_kernel(const uint64_t* __restrict__ keys, uint32_t nt,
                                                             const uint32_t* __restrict__ oldRecs,
                                                             const uint32_t* __restrict__ oldPrimRec,
                                                             uint32_t* __restrict__ recs, uint32_t* __restrict__ primRec) {
    const uint32_t r = blockIdx.x * kLbvhBlock + threadIdx.x;
    if (r >= nt) return;
    const uint32_t prim = (uint32_t)(keys[r] & 0xffffffffull);
    if (prim >= nt) return;
    const uint32_t old = oldPrimRec[prim];
    recs[12 * (size_t)r + 3] = prim;
    recs[12 * (size_t)r + 7] = old < nt ? oldRecs[12 * (size_t)old + 7] : 0u;
    primRec[prim] = r;
}

inline dim3 lanes(uint64_t n) { return dim3((unsigned)((n + kLbvhBlock - 1) / kLbvhBlock)); }

// device allocations of one rebuild: freed at scope exit unless adopted by the scene
struct Allocs {
    std::vector<void*> p;
    ~Allocs() {
        for (void* q : p) (void)hipFree(q);
    }
    hipError_t get(void** out, size_t bytes) {
        const hipError_t e = hipMalloc(out, bytes ? bytes : 256);
        if (e == hipSuccess) p.push_back(*out);
        return e;
    }
    void adopt(void* q) {
        for (void*& x : p)
            if (x == q) x = nullptr;
    }
};

}  // namespace

rsd_status lbvh_rebuild(rsd_scene* s) {
    const uint32_t nt = s->triangle_count, nv = s->vertex_count;
    const uint32_t ni = nt > kLbvhLeaf ? nt - 1u : 0u;  // internal binary nodes that matter: none for a leaf root
    // synchronous: every update and every trace enqueued so far has finished before the tree they read is freed
    RSD_HIP(hipDeviceSynchronize());
    hipStream_t st = nullptr;
    Allocs scratch;
    uint64_t *keysA = nullptr, *keysB = nullptr, *wkeyA = nullptr, *wkeyB = nullptr;
    uint32_t *wvalA = nullptr, *wvalB = nullptr, *first = nullptr, *last = nullptr, *split = nullptr, *parent = nullptr,
             *widx = nullptr, *ctl = nullptr;
    void* tmp = nullptr;
    size_t tmpKeys = 0, tmpPairs = 0;
    if (nt) RSD_HIP(rocprim::radix_sort_keys(nullptr, tmpKeys, keysA, keysB, (size_t)nt, 0u, 62u, st));
    if (ni) RSD_HIP(rocprim::radix_sort_pairs(nullptr, tmpPairs, wkeyA, wkeyB, wvalA, wvalB, (size_t)ni, 0u, kWideKeyBits, st));
    RSD_HIP(scratch.get((void**)&ctl, 4 * (kCtlWords + 6)));
    uint32_t* box = ctl + kCtlWords;
    RSD_HIP(scratch.get((void**)&keysA, 8 * (size_t)nt));
    RSD_HIP(scratch.get((void**)&keysB, 8 * (size_t)nt));
    RSD_HIP(scratch.get((void**)&wkeyA, 8 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&wkeyB, 8 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&wvalA, 4 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&wvalB, 4 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&first, 4 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&last, 4 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&split, 4 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&parent, 4 * (size_t)ni));
    RSD_HIP(scratch.get((void**)&widx, 4 * (size_t)ni));
    RSD_HIP(scratch.get(&tmp, tmpKeys > tmpPairs ? tmpKeys : tmpPairs));

    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    RSD_HIP(hipEventCreate(&ev0));
    if (const hipError_t e = hipEventCreate(&ev1); e != hipSuccess) {
        (void)hipEventDestroy(ev0);
        return hip_fail(e, "rsd_scene_rebuild_bvh: hipEventCreate");
    }
    struct Events {
        hipEvent_t a, b;
        ~Events() {
            (void)hipEventDestroy(a);
            (void)hipEventDestroy(b);
        }
    } events{ev0, ev1};

    const uint32_t* ind = s->dyn.indices;
    const uint32_t* pos = reinterpret_cast<const uint32_t*>(s->dyn.positions);
    RSD_HIP(hipEventRecord(ev0, st));
    RSD_HIP(hipMemsetAsync(ctl, 0, 4 * (kCtlWords + 6), st));
    RSD_HIP(hipMemsetAsync(box, 0xff, 12, st));
    uint32_t ctlHost[kCtlWords] = {0u, 0u, 0u, 0u};
    if (nt) {
        const uint64_t comps = 3ull * nt;
        const unsigned blocks = (unsigned)std::min<uint64_t>((comps + kLbvhBlock - 1) / kLbvhBlock, 2048);
        hipLaunchKernelGGL(scene_box_kernel, dim3(blocks), dim3(kLbvhBlock), 0, st, ind, pos, nv, nt, box);
        if (rsd_status r = launch_status("scene_box_kernel launch"); r != RSD_OK) return r;
        hipLaunchKernelGGL(keys_kernel, lanes(nt), dim3(kLbvhBlock), 0, st, ind, pos, nv, nt, box, keysA);
        if (rsd_status r = launch_status("keys_kernel launch"); r != RSD_OK) return r;
        RSD_HIP(rocprim::radix_sort_keys(tmp, tmpKeys, keysA, keysB, (size_t)nt, 0u, 62u, st));
    }
    if (ni) {
        RSD_HIP(hipMemsetAsync(parent, 0xff, 4 * (size_t)ni, st));
        RSD_HIP(hipMemsetAsync(widx, 0xff, 4 * (size_t)ni, st));
        hipLaunchKernelGGL(karras_kernel, lanes(ni), dim3(kLbvhBlock), 0, st, keysB, nt, first, last, split, parent);
        if (rsd_status r = launch_status("karras_kernel launch"); r != RSD_OK) return r;
        hipLaunchKernelGGL(depth_kernel, lanes(ni), dim3(kLbvhBlock), 0, st, ni, first, last, parent, wkeyA, wvalA, ctl);
        if (rsd_status r = launch_status("depth_kernel launch"); r != RSD_OK) return r;
        RSD_HIP(rocprim::radix_sort_pairs(tmp, tmpPairs, wkeyA, wkeyB, wvalA, wvalB, (size_t)ni, 0u, kWideKeyBits, st));
        RSD_HIP(hipMemcpy(ctlHost, ctl, sizeof(ctlHost), hipMemcpyDeviceToHost));  // waits for the launches above
        if (ctlHost[kCtlWide] == 0u || ctlHost[kCtlWide] > ni || ctlHost[kCtlLevel] + 1u > kLbvhMaxWideDepth) {
            set_error("rsd_scene_rebuild_bvh: the device tree is not one of the definition (" +
                      std::to_string(ctlHost[kCtlWide]) + " wide nodes, level " + std::to_string(ctlHost[kCtlLevel]) + ")");
            return RSD_ERR_HIP;
        }
    }
    const uint32_t nn = ni ? ctlHost[kCtlWide] : 1u;

    // the new tree: nodes + records + pad (rsd_scene_upload's layout), the refit's tables, the primitive map
    Allocs fresh;
    const size_t nodeBytes = 128 * (size_t)nn, bvhBytes = nodeBytes + 48 * (size_t)nt + 12 * 16;
    const DynLayout lay = dyn_layout(nt, nv, nn);
    char *dNodes = nullptr, *dDyn = nullptr;
    uint32_t* dPrimRec = nullptr;
    RSD_HIP(fresh.get((void**)&dNodes, bvhBytes));
    RSD_HIP(fresh.get((void**)&dDyn, lay.total));
    if (nt) RSD_HIP(fresh.get((void**)&dPrimRec, 4 * (size_t)nt));
    RSD_HIP(hipMemsetAsync(dNodes, 0, bvhBytes, st));
    RSD_HIP(hipMemsetAsync(dDyn + lay.parent, 0, lay.total - lay.parent, st));
    // indices and positions keep their offsets: the per-node tables follow them (dyn_layout)
    if (lay.parent) RSD_HIP(hipMemcpyAsync(dDyn, s->d_dyn, lay.parent, hipMemcpyDeviceToDevice, st));
    uint32_t* nodes = reinterpret_cast<uint32_t*>(dNodes);
    uint32_t* recs = reinterpret_cast<uint32_t*>(dNodes + nodeBytes);
    uint32_t* parentOut = reinterpret_cast<uint32_t*>(dDyn + lay.parent);
    uint32_t* innerOut = reinterpret_cast<uint32_t*>(dDyn + lay.inner);
    if (ni) {
        hipLaunchKernelGGL(wide_index_kernel, lanes(nn), dim3(kLbvhBlock), 0, st, nn, ni, wvalB, widx);
        if (rsd_status r = launch_status("wide_index_kernel launch"); r != RSD_OK) return r;
        hipLaunchKernelGGL(wide_kernel, lanes(nn), dim3(kLbvhBlock), 0, st, nn, ni, wvalB, widx, first, last, split, nodes,
                           parentOut, innerOut, ctl);
        if (rsd_status r = launch_status("wide_kernel launch"); r != RSD_OK) return r;
    } else {
        // a leaf root: one node with one leaf slot (none without triangles)
        uint32_t root[8] = {nt ? 0u : kRefitEmptyRef, kRefitEmptyRef, kRefitEmptyRef, kRefitEmptyRef, nt, 0u, 0u, 0u};
        const uint32_t noParent = kRefitNoParent;
        RSD_HIP(hipMemcpyAsync(nodes + 24, root, sizeof(root), hipMemcpyHostToDevice, st));
        RSD_HIP(hipMemcpyAsync(parentOut, &noParent, 4, hipMemcpyHostToDevice, st));
        RSD_HIP(hipStreamSynchronize(st));  // the two sources live on this stack
    }
    if (nt) {
        hipLaunchKernelGGL(records_kernel, lanes(nt), dim3(kLbvhBlock), 0, st, keysB, nt,
                           reinterpret_cast<const uint32_t*>(s->d_tris), s->d_prim_rec, recs, dPrimRec);
        if (rsd_status r = launch_status("records_kernel launch"); r != RSD_OK) return r;
    }
    RSD_HIP(hipStreamSynchronize(st));  // the old tree has been read for the last time

    // swap: from here on the scene owns the new allocations
    void* oldNodes = s->d_nodes;
    void* oldPrimRec = s->d_prim_rec;
    void* oldDyn = s->d_dyn;
    s->device_bytes -= s->bvh_bytes + s->dyn_bytes + (oldPrimRec ? 4 * (uint64_t)nt : 0);
    s->d_nodes = reinterpret_cast<float4*>(dNodes);
    s->tri_offset = 8 * nn;
    s->d_tris = s->d_nodes + s->tri_offset;
    s->node_count = nn;
    s->bvh_bytes = bvhBytes;
    s->d_prim_rec = dPrimRec;
    s->d_dyn = dDyn;
    s->dyn.indices = reinterpret_cast<uint32_t*>(dDyn + lay.indices);
    s->dyn.positions = reinterpret_cast<float*>(dDyn + lay.positions);
    s->dyn.parent = parentOut;
    s->dyn.inner = innerOut;
    s->dyn.arrive = reinterpret_cast<uint32_t*>(dDyn + lay.arrive);
    s->dyn.tight = reinterpret_cast<uint32_t*>(dDyn + lay.tight);
    s->dyn_bytes = lay.total;
    s->device_bytes += bvhBytes + lay.total + (dPrimRec ? 4 * (uint64_t)nt : 0);
    fresh.adopt(dNodes);
    fresh.adopt(dDyn);
    fresh.adopt(dPrimRec);
    (void)hipFree(oldNodes);
    (void)hipFree(oldPrimRec);
    (void)hipFree(oldDyn);
    s->entry_stale = s->entry_stale || s->d_entry != nullptr;

    rsd_status rs = refit_enqueue(s, st);
    hipError_t e = hipEventRecord(ev1, st);
    if (e == hipSuccess) e = hipMemcpy(ctlHost + kCtlLeaves, ctl + kCtlLeaves, 4, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    float ms = 0.0f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev0, ev1);
    s->stats = BvhStats{};
    s->stats.inner_nodes = nn;
    s->stats.leaves = ni ? ctlHost[kCtlLeaves] : (nt ? 1u : 0u);
    s->stats.max_depth = ctlHost[kCtlDepth];
    s->stats.wide_depth = ni ? ctlHost[kCtlLevel] + 1u : 1u;
    s->stats.references = nt;
    s->stats.build_ms = ms;
    s->rebuild_ms = ms;
    if (rs != RSD_OK) return rs;
    if (e != hipSuccess) return hip_fail(e, "rsd_scene_rebuild_bvh");
    ++s->rebuilds;
    return RSD_OK;
}

}  // namespace rsd
