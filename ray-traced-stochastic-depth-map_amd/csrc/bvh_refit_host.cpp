// bvh_refit_host.cpp -- the BVH refit on the host (bvh_refit.h): the byte-exact statement of what the
// kernels of bvh_refit.hip produce, and the topology tables rsd_scene_upload_dynamic keeps on the device.
#include "bvh_refit.h"

#include <cstring>
#include <vector>

namespace rsd {

bool refit_topology(const uint32_t* nodes, uint32_t node_count, uint32_t record_count, uint32_t* parent,
                    uint32_t* inner) {
    for (uint32_t n = 0; n < node_count; ++n) {
        parent[n] = kRefitNoParent;
        inner[n] = 0;
    }
    for (uint32_t n = 0; n < node_count; ++n) {
        const uint32_t* nd = nodes + 32 * (size_t)n;
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t ref = nd[24 + i], cnt = nd[28 + i];
            if (cnt != 0) {
                if (cnt > 4 || ref > record_count || cnt > record_count - ref) return false;
                continue;
            }
            if (ref == kRefitEmptyRef) continue;
            // the collapse numbers a node before its subtree: a child's index is above its parent's, which is
            // what lets refit_host sweep the array backwards
            if (ref >= node_count || ref <= n || parent[ref] != kRefitNoParent) return false;
            parent[ref] = n << 2 | i;
            ++inner[n];
        }
    }
    for (uint32_t n = 1; n < node_count; ++n)
        if (parent[n] == kRefitNoParent) return false;
    return true;
}

void refit_host(uint32_t* bvh, uint32_t node_count, const uint32_t* indices, uint32_t nt, const float* positions) {
    uint32_t* recs = bvh + 32 * (size_t)node_count;
    for (uint32_t r = 0; r < nt; ++r) {
        uint32_t* rec = recs + 12 * (size_t)r;
        const uint32_t prim = rec[0 + 3];
        for (int j = 0; j < 3; ++j)
            std::memcpy(rec + 4 * j, positions + 3 * (size_t)indices[3 * (size_t)prim + j], 12);
    }
    std::vector<RefitBox> tight(node_count);
    for (uint32_t n = node_count; n-- > 0;) {
        uint32_t* nd = bvh + 32 * (size_t)n;
        RefitBox all;
        refit_box_clear(all);
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t ref = nd[24 + i], cnt = nd[28 + i];
            if (cnt == 0 && ref == kRefitEmptyRef) continue;  // empty slots keep their zeros
            RefitBox b;
            if (cnt) {
                refit_box_clear(b);
                refit_box_grow_records(b, recs + 12 * (size_t)ref, cnt);
            } else {
                b = tight[ref];
            }
            refit_store_slot(nd, i, b);
            refit_box_grow(all, b);
        }
        tight[n] = all;
    }
}

}  // namespace rsd
